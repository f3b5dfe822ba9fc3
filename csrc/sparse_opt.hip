// Server-side optimizer step of the sparse handler for CDNA4 (gfx950):
// Adagrad and row-wise Adagrad over the pushed rows of an embedding
// table, with the post-update rows optionally written to a second
// destination in the same pass (the fused ZPushPull round: no gather
// launch, no second read of the table).
//
// Work split, wave64, no LDS. A row belongs to a group of G lanes, G the
// smallest power of two >= the row's vectors (float4, or float on the
// scalar path), at most 64; a wave serves 64 / G rows per step and waves
// take sets of rows in a grid-stride loop. The loop bound is the same for
// every lane of a wave, so lanes without a row or without a column (a
// short last set, a row whose vector count is no power of two, a key
// outside the table) stay in the loop and give zero to the cross-lane
// sum. The gradient row is read once and kept in registers for the
// update (kKeep vectors per lane: rows up to 1024 floats on the float4
// path); vectors past that are read a second time. The row's state is
// read and written by the group's first lane and handed to the others by
// a shuffle. The element-wise variant has no reduction: the same body
// with the shuffles compiled out and the state moved like the table.
//
// Lazy Adam (second half of the file) keeps the lane-group split and
// changes what moves. A row's optimizer state is one record,
//   { p1, p2, v_row, 0 }  m[row_len]  v[row_len] (element-wise only)
// p1 and p2 the running products beta1^t and beta2^t of the row's own
// steps (1 before the first), so a random row costs one DRAM region, not
// three. The group's first lane loads the 16 B header before anything
// else, so its latency hides behind the row's loads; every lane loads its
// resident vectors of gradient, weight and first moment (and second moment,
// element-wise) in one batch ahead of the cross-lane sum, so the update
// that follows the shuffles waits for no memory. The first lane forms p1',
// p2', lr / (1 - p1') and the divisor 1 - p2' (row-wise: the finished
// denominator) once per row, stores the header with one 16 B store, and
// two shuffles hand the per-row scalars to the group: both variants keep
// the wave-uniform loop for them. Vectors past the resident ones stream
// through the update from memory, the gradient read a second time.
// Traffic of a row-wise step with out, by construction: 3L floats in
// (gradient, weight, m) and 3L out (weight, m, out), plus 32 B of header
// (16 B each way); element-wise adds L in and L out for v.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "kernels.h"
#include "sparse_elem.h"

namespace xps {
namespace kern {

namespace {

constexpr int kKeep = 4;  // gradient vectors a lane keeps between the two passes

__device__ inline float SumSq(float v) { return v * v; }
__device__ inline float SumSq(float4 v) { return v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w; }

// new weights of one vector given a ready denominator (row-wise); Step,
// Denom and the lazy-Adam rules are sparse_elem.h's
__device__ inline float Update(float w, float g, float lr, float denom) {
  return Step(w, g, lr, denom);
}
__device__ inline float4 Update(float4 w, float4 g, float lr, float denom) {
  return float4{Step(w.x, g.x, lr, denom), Step(w.y, g.y, lr, denom), Step(w.z, g.z, lr, denom),
                Step(w.w, g.w, lr, denom)};
}

// element-wise: *s += g * g, then the step under the element's own state
__device__ inline float UpdateElem(float w, float g, float* s, float lr, float eps) {
  *s += g * g;
  return Step(w, g, lr, Denom(*s, eps));
}
__device__ inline float4 UpdateElem(float4 w, float4 g, float4* s, float lr, float eps) {
  return float4{UpdateElem(w.x, g.x, &s->x, lr, eps), UpdateElem(w.y, g.y, &s->y, lr, eps),
                UpdateElem(w.z, g.z, &s->z, lr, eps), UpdateElem(w.w, g.w, &s->w, lr, eps)};
}

struct AdagradArgs {
  const uint64_t* rows;
  size_t nrows;
  size_t nv;      // vectors per row
  float row_len;  // floats per row: the divisor of the row-wise mean
  float lr;
  float eps;
  int log2g;  // G = 1 << log2g lanes per row
  int shift;
  uint64_t base;
  uint64_t tab_rows;
};

template <class V, bool kRowwise>
__global__ void __launch_bounds__(kBlock)
    sparse_adagrad_kernel(V* __restrict__ table, float* __restrict__ state,
                          const V* __restrict__ grad, V* __restrict__ out, AdagradArgs a) {
  const int G = 1 << a.log2g;
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1);  // lane within the row's group
  const size_t rows_per_wave = 64 >> a.log2g;
  const size_t tid = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  const size_t wave = tid >> 6;
  const size_t nwaves = (static_cast<size_t>(gridDim.x) * blockDim.x) >> 6;
  const size_t nv = a.nv;
  const size_t resident = static_cast<size_t>(kKeep) << a.log2g;  // vectors the registers hold
  const V zero{};

  // wave-uniform bounds: every lane of the wave reaches the shuffles
  for (size_t first = wave * rows_per_wave; first < a.nrows; first += nwaves * rows_per_wave) {
    const size_t r = first + (lane >> a.log2g);
    const bool live = r < a.nrows;
    const uint64_t row = live ? (a.rows[r] >> a.shift) - a.base : ~0ull;
    const bool ok = live && row < a.tab_rows;  // unsigned: also catches keys below base
    const V* gp = grad + (live ? r * nv : 0);
    V* tp = table + (ok ? row * nv : 0);

    V g[kKeep];
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < kKeep; ++k) {
      const size_t c = gl + (static_cast<size_t>(k) << a.log2g);
      g[k] = (ok && c < nv) ? gp[c] : zero;
      if (kRowwise) ss += SumSq(g[k]);
    }

    float denom = 0.f;
    if (kRowwise) {
      if (ok) {
        for (size_t c = resident + gl; c < nv; c += G) ss += SumSq(gp[c]);
      }
      for (int m = G >> 1; m > 0; m >>= 1) ss += __shfl_xor(ss, m);
      float s = 0.f;
      if (ok && gl == 0) {
        s = state[row] + ss / a.row_len;
        state[row] = s;
      }
      s = __shfl(s, lane - gl);
      denom = Denom(s, a.eps);
    }

    if (!live) continue;  // past the shuffles: nothing below crosses lanes
    if (!ok) {
      // the gather's defined output for a key outside the table
      if (out) {
        for (size_t c = gl; c < nv; c += G) out[r * nv + c] = zero;
      }
      continue;
    }
    V* sp = kRowwise ? nullptr : reinterpret_cast<V*>(state) + row * nv;
    auto apply = [&](size_t c, V gv) {
      V w;
      if (kRowwise) {
        w = Update(tp[c], gv, a.lr, denom);
      } else {
        V s = sp[c];
        w = UpdateElem(tp[c], gv, &s, a.lr, a.eps);
        sp[c] = s;
      }
      tp[c] = w;
      if (out) out[r * nv + c] = w;
    };
#pragma unroll
    for (int k = 0; k < kKeep; ++k) {
      const size_t c = gl + (static_cast<size_t>(k) << a.log2g);
      if (c < nv) apply(c, g[k]);
    }
    for (size_t c = resident + gl; c < nv; c += G) apply(c, gp[c]);
  }
}

template <class V, bool kRowwise>
void LaunchAdagrad(float* table, float* state, const float* grad, float* out, AdagradArgs a,
                   int grid_cap, hipStream_t s) {
  while ((size_t{1} << a.log2g) < a.nv && a.log2g < 6) ++a.log2g;
  size_t rows_per_wave = 64 >> a.log2g;
  size_t waves = (a.nrows + rows_per_wave - 1) / rows_per_wave;
  // the sparse kernels' grid: enough blocks for the 8 XCDs, at most 16384
  int grid = GridFor(waves * 64, 16384, grid_cap);
  hipLaunchKernelGGL((sparse_adagrad_kernel<V, kRowwise>), dim3(grid), dim3(kBlock), 0, s,
                     reinterpret_cast<V*>(table), state, reinterpret_cast<const V*>(grad),
                     reinterpret_cast<V*>(out), a);
}

// ------------------------------------------------------------ lazy Adam
//
// The exact order of the fp32 operations, one IEEE rounding each. The
// moments' multiply-adds are compiled uncontracted (sparse_elem.h); the one
// product left next to a subtraction is p' in 1 - p', where the compiler may
// use the unrounded p * beta (the tests' bound allows for both).
// omb1 and omb2 are the fp32 values of 1 - beta1 and 1 - beta2, formed on
// the host.
//   per row, by the group's first lane:
//     p1' = p1 * beta1                 p2' = p2 * beta2
//     alpha = lr / (1 - p1')           c2 = 1 - p2'
//   row-wise only, also per row:
//     ss = sum of g * g over the row (any order), mean = ss / row_len
//     v' = beta2 * v_row + omb2 * mean         multiply, multiply, add
//     denom = sqrt(v' / c2) + eps              divide, square root, add
//   per element:
//     m' = beta1 * m + omb1 * g                multiply, multiply, add
//     element-wise only:
//       v' = beta2 * v + omb2 * (g * g)        three multiplies, one add
//       denom = sqrt(v' / c2) + eps            divide, square root, add
//     w' = w - (alpha * m') / denom            multiply, divide, subtract
// A fresh row (p = 1, m = v = 0) with a zero gradient has m' = v' = 0, the
// step is 0 / eps = 0 and w keeps its bits: the reason eps must be > 0.

struct LazyAdamArgs {
  const uint64_t* rows;
  size_t nrows;
  size_t nv;      // vectors per row
  size_t rec;     // floats per state record
  float row_len;  // floats per row: the divisor of the row-wise mean
  float lr;
  float beta1, beta2;
  float omb1, omb2;  // 1 - beta1, 1 - beta2
  float eps;
  int log2g;  // G = 1 << log2g lanes per row
  int shift;
  uint64_t base;
  uint64_t tab_rows;
};

// One element's update. q is the row's denominator (row-wise; *v unused) or
// its divisor c2 (element-wise).
template <bool kRowwise>
__device__ inline void AdamElem(float* w, float* m, float* v, float g, float alpha, float q,
                                const LazyAdamArgs& a) {
  *m = Moment(*m, g, a.beta1, a.omb1);
  float denom = q;
  if (!kRowwise) {
    *v = Moment(*v, g * g, a.beta2, a.omb2);
    denom = AdamDenom(*v, q, a.eps);
  }
  *w = AdamStep(*w, *m, alpha, denom);
}
template <bool kRowwise>
__device__ inline void AdamElem(float4* w, float4* m, float4* v, float4 g, float alpha, float q,
                                const LazyAdamArgs& a) {
  AdamElem<kRowwise>(&w->x, &m->x, &v->x, g.x, alpha, q, a);
  AdamElem<kRowwise>(&w->y, &m->y, &v->y, g.y, alpha, q, a);
  AdamElem<kRowwise>(&w->z, &m->z, &v->z, g.z, alpha, q, a);
  AdamElem<kRowwise>(&w->w, &m->w, &v->w, g.w, alpha, q, a);
}

template <class V, bool kRowwise>
__global__ void __launch_bounds__(kBlock)
    sparse_lazy_adam_kernel(V* __restrict__ table, float* __restrict__ state,
                            const V* __restrict__ grad, V* __restrict__ out, LazyAdamArgs a) {
  constexpr bool kVec = sizeof(V) == 16;
  constexpr int kHdr = 16 / sizeof(V);      // the header in vectors
  constexpr int kV = kRowwise ? 1 : kKeep;  // resident second-moment vectors
  const int G = 1 << a.log2g;
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1);  // lane within the row's group
  const size_t rows_per_wave = 64 >> a.log2g;
  const size_t tid = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  const size_t wave = tid >> 6;
  const size_t nwaves = (static_cast<size_t>(gridDim.x) * blockDim.x) >> 6;
  const size_t nv = a.nv;
  const size_t resident = static_cast<size_t>(kKeep) << a.log2g;  // vectors the registers hold
  const V zero{};

  // wave-uniform bounds: every lane of the wave reaches the shuffles
  for (size_t first = wave * rows_per_wave; first < a.nrows; first += nwaves * rows_per_wave) {
    const size_t r = first + (lane >> a.log2g);
    const bool live = r < a.nrows;
    const uint64_t row = live ? (a.rows[r] >> a.shift) - a.base : ~0ull;
    const bool ok = live && row < a.tab_rows;  // unsigned: also catches keys below base
    const bool lead = ok && gl == 0;
    const V* gp = grad + (live ? r * nv : 0);
    V* tp = table + (ok ? row * nv : 0);
    float* rec = state + (ok ? row * a.rec : 0);
    V* mp = reinterpret_cast<V*>(rec) + kHdr;
    V* vp = mp + nv;  // element-wise only

    // the header first, then every resident vector of the row in one batch
    float4 h{1.f, 1.f, 0.f, 0.f};
    if (lead) h = LoadHeader<kVec>(rec);
    V g[kKeep], w[kKeep], m[kKeep], v[kV] = {};
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < kKeep; ++k) {
      const size_t c = gl + (static_cast<size_t>(k) << a.log2g);
      const bool has = ok && c < nv;
      g[k] = has ? gp[c] : zero;
      w[k] = has ? tp[c] : zero;
      m[k] = has ? mp[c] : zero;
      if (!kRowwise) v[kRowwise ? 0 : k] = has ? vp[c] : zero;
      if (kRowwise) ss += SumSq(g[k]);
    }
    if (kRowwise) {
      if (ok) {
        for (size_t c = resident + gl; c < nv; c += G) ss += SumSq(gp[c]);
      }
      for (int x = G >> 1; x > 0; x >>= 1) ss += __shfl_xor(ss, x);
    }

    // the row's scalars: alpha, and q = the denominator (row-wise) or c2
    float alpha = 0.f, q = 1.f;
    if (lead) {
      h.x = h.x * a.beta1;
      h.y = h.y * a.beta2;
      alpha = a.lr / (1.f - h.x);
      q = 1.f - h.y;
      if (kRowwise) {
        h.z = Moment(h.z, ss / a.row_len, a.beta2, a.omb2);
        q = AdamDenom(h.z, q, a.eps);
      }
      StoreHeader<kVec>(rec, h);
    }
    alpha = __shfl(alpha, lane - gl);
    q = __shfl(q, lane - gl);

    if (!live) continue;  // past the shuffles: nothing below crosses lanes
    if (!ok) {
      // the gather's defined output for a key outside the table
      if (out) {
        for (size_t c = gl; c < nv; c += G) out[r * nv + c] = zero;
      }
      continue;
    }
    auto apply = [&](size_t c, V gv, V wv, V mv, V vv) {
      AdamElem<kRowwise>(&wv, &mv, &vv, gv, alpha, q, a);
      tp[c] = wv;
      mp[c] = mv;
      if (!kRowwise) vp[c] = vv;
      if (out) out[r * nv + c] = wv;
    };
#pragma unroll
    for (int k = 0; k < kKeep; ++k) {
      const size_t c = gl + (static_cast<size_t>(k) << a.log2g);
      if (c < nv) apply(c, g[k], w[k], m[k], v[kRowwise ? 0 : k]);
    }
    for (size_t c = resident + gl; c < nv; c += G) {
      apply(c, gp[c], tp[c], mp[c], kRowwise ? zero : vp[c]);
    }
  }
}

template <class V, bool kRowwise>
void LaunchLazyAdam(float* table, float* state, const float* grad, float* out, LazyAdamArgs a,
                    int grid_cap, hipStream_t s) {
  while ((size_t{1} << a.log2g) < a.nv && a.log2g < 6) ++a.log2g;
  size_t rows_per_wave = 64 >> a.log2g;
  size_t waves = (a.nrows + rows_per_wave - 1) / rows_per_wave;
  int grid = GridFor(waves * 64, 16384, grid_cap);
  hipLaunchKernelGGL((sparse_lazy_adam_kernel<V, kRowwise>), dim3(grid), dim3(kBlock), 0, s,
                     reinterpret_cast<V*>(table), state, reinterpret_cast<const V*>(grad),
                     reinterpret_cast<V*>(out), a);
}

}  // namespace

void SparseAdagradF32(float* table, float* state, const uint64_t* rows_dev, size_t nrows,
                      size_t row_len, const float* grad, float* out_or_null, float lr, float eps,
                      bool rowwise, hipStream_t s, int key_shift, uint64_t row_base,
                      uint64_t table_rows, int grid_cap) {
  if (!(lr > 0.f)) throw std::invalid_argument("SparseAdagradF32: lr must be positive");
  if (!(eps > 0.f)) throw std::invalid_argument("SparseAdagradF32: eps must be positive");
  if (nrows == 0 || row_len == 0) return;
  AdagradArgs a{};
  a.rows = rows_dev;
  a.nrows = nrows;
  a.nv = row_len;
  a.row_len = static_cast<float>(row_len);
  a.lr = lr;
  a.eps = eps;
  a.shift = key_shift;
  a.base = row_base;
  a.tab_rows = table_rows;
  // float4 needs whole vectors and every array it moves on a 16 B boundary
  // (the row-wise state moves as single floats)
  bool vec = row_len % 4 == 0 && Aligned16(table, grad, out_or_null) &&
             (rowwise || Aligned16(state));
  if (vec) {
    a.nv = row_len / 4;
    if (rowwise) {
      LaunchAdagrad<float4, true>(table, state, grad, out_or_null, a, grid_cap, s);
    } else {
      LaunchAdagrad<float4, false>(table, state, grad, out_or_null, a, grid_cap, s);
    }
  } else if (rowwise) {
    LaunchAdagrad<float, true>(table, state, grad, out_or_null, a, grid_cap, s);
  } else {
    LaunchAdagrad<float, false>(table, state, grad, out_or_null, a, grid_cap, s);
  }
}

size_t SparseLazyAdamStateFloats(size_t rows, size_t row_len, bool rowwise) {
  return rows * (4 + row_len * (rowwise ? 1 : 2));
}

void SparseLazyAdamF32(float* table, float* state, const uint64_t* rows_dev, size_t nrows,
                       size_t row_len, const float* grad, float* out_or_null, float lr, float beta1,
                       float beta2, float eps, bool rowwise, hipStream_t s, int key_shift,
                       uint64_t row_base, uint64_t table_rows, int grid_cap) {
  if (!(lr > 0.f)) throw std::invalid_argument("SparseLazyAdamF32: lr must be positive");
  if (!(eps > 0.f)) throw std::invalid_argument("SparseLazyAdamF32: eps must be positive");
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) {
    throw std::invalid_argument("SparseLazyAdamF32: beta1 and beta2 must lie in [0, 1)");
  }
  // every record's header is one 16 B access on the float4 path
  if (!Aligned16(state)) {
    throw std::invalid_argument("SparseLazyAdamF32: state must be 16 B-aligned");
  }
  if (nrows == 0 || row_len == 0) return;
  LazyAdamArgs a{};
  a.rows = rows_dev;
  a.nrows = nrows;
  a.nv = row_len;
  a.rec = SparseLazyAdamStateFloats(1, row_len, rowwise);
  a.row_len = static_cast<float>(row_len);
  a.lr = lr;
  a.beta1 = beta1;
  a.beta2 = beta2;
  a.omb1 = 1.f - beta1;
  a.omb2 = 1.f - beta2;
  a.eps = eps;
  a.shift = key_shift;
  a.base = row_base;
  a.tab_rows = table_rows;
  // float4 needs whole vectors and every array it moves on a 16 B boundary;
  // the records then are, since their length is a multiple of four floats
  if (row_len % 4 == 0 && Aligned16(table, grad, out_or_null)) {
    a.nv = row_len / 4;
    if (rowwise) {
      LaunchLazyAdam<float4, true>(table, state, grad, out_or_null, a, grid_cap, s);
    } else {
      LaunchLazyAdam<float4, false>(table, state, grad, out_or_null, a, grid_cap, s);
    }
  } else if (rowwise) {
    LaunchLazyAdam<float, true>(table, state, grad, out_or_null, a, grid_cap, s);
  } else {
    LaunchLazyAdam<float, false>(table, state, grad, out_or_null, a, grid_cap, s);
  }
}

}  // namespace kern
}  // namespace xps
