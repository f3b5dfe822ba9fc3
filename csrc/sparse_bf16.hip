// The sparse handler's kernels over a bf16 embedding table for CDNA4
// (gfx950): gather, assign, add, and the Adagrad and lazy-Adam steps of
// sparse_opt.hip with the weights stored as bf16 bits. The optimizer state
// stays fp32; a step widens the weight exactly, runs sparse_elem.h's fp32
// arithmetic unchanged, and rounds once on the store. The wire side (the
// gradients and pushed values, the returned rows) is fp32 (Sparse*Bf16) or
// bf16 bits (Sparse*Bf16Wire): a 16-bit gradient is widened exactly and a
// 16-bit row out is the stored bits, so the two wires leave the same table
// and state bits for the same values.
//
// The store rule R(x), u the bits of x: nearest is round-to-nearest-even;
// stochastic stores (u + r) >> 16 with r uniform in [0, 2^16), so the
// magnitude goes up with probability (u & 0xffff) / 2^16 and a value that
// already is a bf16 keeps its bits whatever r is. Inf and NaN pass through
// both (a NaN keeps a mantissa bit). r is a field of a counter-based 64-bit
// word: SplitMix64 seeded per row,
//   row_key = mix(seed + (row + 1) * phi)          row = the local table row
//   word(q) = mix(row_key + (q + 1) * phi)         q = element index / 4
//   r       = (word >> 16 * (element index % 4)) & 0xffff
// phi = 0x9E3779B97F4A7C15 and mix the SplitMix64 finalizer. No state, no
// dependence on lanes, waves or the grid: the same call gives the same bits
// on the vector and the scalar path and under any grid_cap.
//
// Work split of the steps, wave64, no LDS. The arrays of a row differ in
// width, so a lane's unit is 8 elements: one 16 B access of the table
// against two float4 each of gradient, moments and out. A row belongs to a
// group of G lanes, G the smallest power of two >= row_len / 8, at most 64;
// a wave serves 64 / G rows per pass and waves take sets of rows in a
// grid-stride loop whose bound is wave-uniform, so every lane reaches the
// shuffles. Each lane loads its kKeep resident units of every array in one
// batch (the weights stay packed, 4 registers per unit) ahead of the
// cross-lane sum; the group's first lane forms the row's scalars, and the
// lazy-Adam header, once and shuffles hand them out. Rows past
// kKeep * 64 * 8 = 1024 elements stream the rest, the gradient read a second
// time. The scalar path (row_len % 8 != 0 or a pointer off its 16 B
// boundary) is the same body with a unit of one element, uint16_t against
// float, for the whole call.
// With a 16-bit wire every row array of a unit is one 16 B access, and a
// resident gradient unit stays packed, 4 registers, until its row's scalars
// are known; the scalar path moves uint16_t against uint16_t.
// Traffic per row of L elements, by construction: row-wise Adagrad with out
// 12 L bytes (fp32 table: 16 L; 16-bit wire: 8 L), row-wise lazy Adam
// 20 L + 32 (24 L + 32; 16 L + 32), gather 6 L (8 L; 4 L).
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <type_traits>

#include "kernels.h"
#include "sparse_elem.h"

namespace xps {
namespace kern {

namespace {

// resident units of a lane: 16 elements of each array. 4 was measured for the
// 16-bit wire's smaller gradient unit (profiles/sparse_bf16_wire.md): faster
// at row length 2048, slower at 64 on both wires, so it stays 2.
constexpr int kKeep = 2;
constexpr uint64_t kPhi = 0x9E3779B97F4A7C15ull;

__host__ __device__ inline uint64_t Mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// how a launch rounds; nearest leaves row_key unused
struct Rounding {
  uint64_t seed;
  int stochastic;
};
__device__ inline uint64_t RowKey(const Rounding& rd, uint64_t row) {
  return Mix64(rd.seed + (row + 1) * kPhi);
}

__device__ inline uint16_t RoundBf16(float x, uint32_t r16, bool stochastic) {
  uint32_t u = __float_as_uint(x);
  uint32_t h = u >> 16;
  if ((u & 0x7f800000u) == 0x7f800000u) {
    // Inf as it is; a NaN whose mantissa lies in the dropped half keeps a bit
    if ((h & 0x7fu) == 0 && (u & 0xffffu)) h |= 0x40u;
    return static_cast<uint16_t>(h);
  }
  uint32_t add = stochastic ? r16 : 0x7fffu + (h & 1u);
  return static_cast<uint16_t>((u + add) >> 16);
}
__device__ inline float Widen(uint32_t bits) { return __uint_as_float(bits << 16); }

// a unit of kN elements: the table's packed form and its accesses
template <int kN>
struct Unit;
template <>
struct Unit<8> {
  using Packed = uint4;
  static __device__ inline void Unpack(uint4 p, float (&x)[8]) {
    const uint32_t w[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x[2 * i] = __uint_as_float(w[i] << 16);
      x[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
  static __device__ inline uint4 Pack(const uint16_t (&b)[8]) {
    return uint4{b[0] | (uint32_t{b[1]} << 16), b[2] | (uint32_t{b[3]} << 16),
                 b[4] | (uint32_t{b[5]} << 16), b[6] | (uint32_t{b[7]} << 16)};
  }
  static __device__ inline uint4 LoadW(const uint16_t* p) {
    return *reinterpret_cast<const uint4*>(p);
  }
  static __device__ inline void StoreW(uint16_t* p, uint4 v) { *reinterpret_cast<uint4*>(p) = v; }
  static __device__ inline void LoadF(const float* p, float (&x)[8]) {
    const float4 a = reinterpret_cast<const float4*>(p)[0];
    const float4 b = reinterpret_cast<const float4*>(p)[1];
    x[0] = a.x, x[1] = a.y, x[2] = a.z, x[3] = a.w;
    x[4] = b.x, x[5] = b.y, x[6] = b.z, x[7] = b.w;
  }
  static __device__ inline void StoreF(float* p, const float (&x)[8]) {
    reinterpret_cast<float4*>(p)[0] = float4{x[0], x[1], x[2], x[3]};
    reinterpret_cast<float4*>(p)[1] = float4{x[4], x[5], x[6], x[7]};
  }
};
template <>
struct Unit<1> {
  using Packed = uint16_t;
  static __device__ inline void Unpack(uint16_t p, float (&x)[1]) { x[0] = Widen(p); }
  static __device__ inline uint16_t Pack(const uint16_t (&b)[1]) { return b[0]; }
  static __device__ inline uint16_t LoadW(const uint16_t* p) { return *p; }
  static __device__ inline void StoreW(uint16_t* p, uint16_t v) { *p = v; }
  static __device__ inline void LoadF(const float* p, float (&x)[1]) { x[0] = *p; }
  static __device__ inline void StoreF(float* p, const float (&x)[1]) { *p = x[0]; }
};

// The wire side of a unit: the gradient or pushed values in, the rows out.
// Held is what a lane keeps of a unit it has loaded, Open its fp32 values;
// Store writes a unit of rows out, given both its values x and their bits.
template <int kN>
struct F32Wire {
  using T = float;
  struct Held {
    float x[kN];
  };
  static __device__ inline Held Load(const float* p) {
    Held h;
    Unit<kN>::LoadF(p, h.x);
    return h;
  }
  static __device__ inline void Open(const Held& h, float (&x)[kN]) {
#pragma unroll
    for (int j = 0; j < kN; ++j) x[j] = h.x[j];
  }
  static __device__ inline void Store(float* p, const float (&x)[kN], typename Unit<kN>::Packed) {
    Unit<kN>::StoreF(p, x);
  }
};
template <int kN>
struct Bf16Wire {
  using T = uint16_t;
  using Held = typename Unit<kN>::Packed;
  static __device__ inline Held Load(const uint16_t* p) { return Unit<kN>::LoadW(p); }
  static __device__ inline void Open(Held h, float (&x)[kN]) { Unit<kN>::Unpack(h, x); }
  static __device__ inline void Store(uint16_t* p, const float (&)[kN], Held bits) {
    Unit<kN>::StoreW(p, bits);
  }
};
// the two wires by the type of their arrays
template <class T, int kN>
using WireOf = std::conditional_t<std::is_same<T, float>::value, F32Wire<kN>, Bf16Wire<kN>>;

// R over unit c of a row: the packed bits to store, x left as those bits
// widened (what a later gather returns)
template <int kN>
__device__ inline typename Unit<kN>::Packed Round(float (&x)[kN], size_t c, uint64_t row_key,
                                                  bool stochastic) {
  uint16_t b[kN];
  uint64_t word = 0;
#pragma unroll
  for (int j = 0; j < kN; ++j) {
    const size_t e = c * kN + j;  // the element's index in its row
    if (stochastic && (kN == 1 || j % 4 == 0)) word = Mix64(row_key + ((e >> 2) + 1) * kPhi);
    b[j] = RoundBf16(x[j], static_cast<uint32_t>(word >> (16 * (e & 3))) & 0xffffu, stochastic);
    x[j] = Widen(b[j]);
  }
  return Unit<kN>::Pack(b);
}

template <int kN>
__device__ inline void Zero(float (&x)[kN]) {
#pragma unroll
  for (int j = 0; j < kN; ++j) x[j] = 0.f;
}

// ------------------------------------------------- gather, assign, add

enum class Move { kGather, kAssign, kAdd };

struct MoveArgs {
  const uint64_t* rows;
  size_t nrows;
  size_t nv;  // units per row
  int shift;
  uint64_t base;
  uint64_t tab_rows;
  Rounding rd;
};

// one unit of one message row per lane and step, grid-stride; f is the wire
// side: out (gather), src (assign, add). A 16-bit gather and assign move
// bits: the worker rounded what it assigns.
template <int kN, Move kOp, class T>
__global__ void __launch_bounds__(kBlock)
    sparse_move_bf16_kernel(uint16_t* __restrict__ table, T* __restrict__ f, MoveArgs a) {
  using U = Unit<kN>;
  using W = WireOf<T, kN>;
  using Packed = typename U::Packed;
  const size_t total = a.nrows * a.nv;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; i < total;
       i += stride) {
    const size_t r = i / a.nv, c = i - r * a.nv;
    const uint64_t row = (a.rows[r] >> a.shift) - a.base;
    const bool ok = row < a.tab_rows;  // unsigned: also catches keys below base
    float x[kN];
    if (!ok) {
      if (kOp == Move::kGather) {
        Zero(x);
        W::Store(f + i * kN, x, Packed{});
      }
      continue;
    }
    uint16_t* tp = table + (row * a.nv + c) * kN;
    if (kOp == Move::kGather) {
      const Packed p = U::LoadW(tp);
      U::Unpack(p, x);
      W::Store(f + i * kN, x, p);
      continue;
    }
    const typename W::Held h = W::Load(f + i * kN);
    if constexpr (kOp == Move::kAssign && std::is_same<T, uint16_t>::value) {
      U::StoreW(tp, h);
      continue;
    }
    W::Open(h, x);
    if (kOp == Move::kAdd) {
      float w[kN];
      U::Unpack(U::LoadW(tp), w);
#pragma unroll
      for (int j = 0; j < kN; ++j) x[j] = w[j] + x[j];
    }
    const bool stochastic = kOp == Move::kAdd && a.rd.stochastic;
    U::StoreW(tp, Round<kN>(x, c, stochastic ? RowKey(a.rd, row) : 0, stochastic));
  }
}

template <Move kOp, class T>
void LaunchMove(uint16_t* table, T* f, size_t row_len, MoveArgs a, int grid_cap, hipStream_t s) {
  if (a.nrows == 0 || row_len == 0) return;
  const bool vec = row_len % 8 == 0 && Aligned16(table) && Aligned16(f);
  a.nv = vec ? row_len / 8 : row_len;
  int grid = GridFor(a.nrows * a.nv, 16384, grid_cap);
  if (vec) {
    hipLaunchKernelGGL((sparse_move_bf16_kernel<8, kOp, T>), dim3(grid), dim3(kBlock), 0, s, table,
                       f, a);
  } else {
    hipLaunchKernelGGL((sparse_move_bf16_kernel<1, kOp, T>), dim3(grid), dim3(kBlock), 0, s, table,
                       f, a);
  }
}

MoveArgs MakeMove(const uint64_t* rows, size_t nrows, int key_shift, uint64_t row_base,
                  uint64_t table_rows, Bf16Rounding rounding, uint64_t seed) {
  MoveArgs a{};
  a.rows = rows;
  a.nrows = nrows;
  a.shift = key_shift;
  a.base = row_base;
  a.tab_rows = table_rows;
  a.rd = Rounding{seed, rounding == Bf16Rounding::kStochastic};
  return a;
}

// ------------------------------------------------------ optimizer steps

struct StepArgs {
  const uint64_t* rows;
  size_t nrows;
  size_t nv;      // units per row
  size_t rec;     // lazy Adam: floats per state record
  float row_len;  // elements per row: the divisor of the row-wise mean
  float lr;
  float beta1, beta2;
  float omb1, omb2;  // 1 - beta1, 1 - beta2
  float eps;
  int log2g;  // G = 1 << log2g lanes per row
  int shift;
  uint64_t base;
  uint64_t tab_rows;
  Rounding rd;
};

template <int kN>
__device__ inline float SumSq(const float (&g)[kN]) {
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < kN; ++j) ss += g[j] * g[j];
  return ss;
}
template <class W, int kN>
__device__ inline float SumSqOf(const typename W::Held& h) {
  float g[kN];
  W::Open(h, g);
  return SumSq(g);
}

// what a lane knows of its row in one pass of the wave's loop
struct RowAt {
  size_t r;      // the message row
  uint64_t row;  // the local table row
  bool live;     // r is a row of the message
  bool ok;       // and row lies in the table
};
__device__ inline RowAt Locate(const StepArgs& a, size_t first, int lane) {
  RowAt at;
  at.r = first + (lane >> a.log2g);
  at.live = at.r < a.nrows;
  at.row = at.live ? (a.rows[at.r] >> a.shift) - a.base : ~0ull;
  at.ok = at.live && at.row < a.tab_rows;  // unsigned: also catches keys below base
  return at;
}

// the gather's defined output for a key outside the table
template <class W, int kN>
__device__ inline void ZeroRow(typename W::T* out, size_t nv, int gl, int G) {
  float z[kN];
  Zero(z);
  for (size_t c = gl; c < nv; c += G) W::Store(out + c * kN, z, typename Unit<kN>::Packed{});
}

template <int kN, bool kRowwise, class T>
__global__ void __launch_bounds__(kBlock)
    sparse_adagrad_bf16_kernel(uint16_t* __restrict__ table, float* __restrict__ state,
                               const T* __restrict__ grad, T* __restrict__ out, StepArgs a) {
  using U = Unit<kN>;
  using W = WireOf<T, kN>;
  using Packed = typename U::Packed;
  using Held = typename W::Held;
  const int G = 1 << a.log2g;
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1);  // lane within the row's group
  const size_t rows_per_wave = 64 >> a.log2g;
  const size_t tid = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  const size_t wave = tid >> 6;
  const size_t nwaves = (static_cast<size_t>(gridDim.x) * blockDim.x) >> 6;
  const size_t nv = a.nv, len = a.nv * kN;
  const size_t resident = static_cast<size_t>(kKeep) << a.log2g;  // units the registers hold

  // wave-uniform bounds: every lane of the wave reaches the shuffles
  for (size_t first = wave * rows_per_wave; first < a.nrows; first += nwaves * rows_per_wave) {
    const RowAt at = Locate(a, first, lane);
    const T* gp = grad + (at.live ? at.r * len : 0);
    uint16_t* tp = table + (at.ok ? at.row * len : 0);
    float* sp = kRowwise ? nullptr : state + (at.ok ? at.row * len : 0);

    // every resident unit of the row in one batch
    Held g[kKeep] = {};
    float st[kRowwise ? 1 : kKeep][kN];
    Packed w[kKeep] = {};
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < kKeep; ++k) {
      const size_t c = gl + (static_cast<size_t>(k) << a.log2g);
      if (at.ok && c < nv) {
        g[k] = W::Load(gp + c * kN);
        w[k] = U::LoadW(tp + c * kN);
        if (!kRowwise) U::LoadF(sp + c * kN, st[kRowwise ? 0 : k]);
      }
      if (kRowwise) ss += SumSqOf<W, kN>(g[k]);
    }

    float denom = 0.f;
    if (kRowwise) {
      if (at.ok) {
        for (size_t c = resident + gl; c < nv; c += G) ss += SumSqOf<W, kN>(W::Load(gp + c * kN));
      }
      for (int m = G >> 1; m > 0; m >>= 1) ss += __shfl_xor(ss, m);
      float s = 0.f;
      if (at.ok && gl == 0) {
        s = state[at.row] + ss / a.row_len;
        state[at.row] = s;
      }
      s = __shfl(s, lane - gl);
      denom = Denom(s, a.eps);
    }

    if (!at.live) continue;  // past the shuffles: nothing below crosses lanes
    T* op = out ? out + at.r * len : nullptr;
    if (!at.ok) {
      if (out) ZeroRow<W, kN>(op, nv, gl, G);
      continue;
    }
    const uint64_t row_key = a.rd.stochastic ? RowKey(a.rd, at.row) : 0;
    auto apply = [&](size_t c, const Held& gh, Packed wv, float (&sv)[kN]) {
      float x[kN], gv[kN];
      W::Open(gh, gv);
      U::Unpack(wv, x);
#pragma unroll
      for (int j = 0; j < kN; ++j) {
        if (kRowwise) {
          x[j] = Step(x[j], gv[j], a.lr, denom);
        } else {
          sv[j] += gv[j] * gv[j];
          x[j] = Step(x[j], gv[j], a.lr, Denom(sv[j], a.eps));
        }
      }
      if (!kRowwise) U::StoreF(sp + c * kN, sv);
      const Packed bits = Round<kN>(x, c, row_key, a.rd.stochastic);
      U::StoreW(tp + c * kN, bits);
      if (out) W::Store(op + c * kN, x, bits);
    };
#pragma unroll
    for (int k = 0; k < kKeep; ++k) {
      const size_t c = gl + (static_cast<size_t>(k) << a.log2g);
      if (c < nv) apply(c, g[k], w[k], st[kRowwise ? 0 : k]);
    }
    for (size_t c = resident + gl; c < nv; c += G) {
      float sv[kN];
      const Held gh = W::Load(gp + c * kN);
      if (!kRowwise) U::LoadF(sp + c * kN, sv);
      apply(c, gh, U::LoadW(tp + c * kN), sv);
    }
  }
}

// The operations and their order are sparse_opt.hip's lazy Adam; the record
// layout is SparseLazyAdamF32's.
template <int kN, bool kRowwise, class T>
__global__ void __launch_bounds__(kBlock)
    sparse_lazy_adam_bf16_kernel(uint16_t* __restrict__ table, float* __restrict__ state,
                                 const T* __restrict__ grad, T* __restrict__ out, StepArgs a) {
  using U = Unit<kN>;
  using W = WireOf<T, kN>;
  using Packed = typename U::Packed;
  using Held = typename W::Held;
  constexpr bool kVec = kN == 8;
  const int G = 1 << a.log2g;
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1);  // lane within the row's group
  const size_t rows_per_wave = 64 >> a.log2g;
  const size_t tid = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  const size_t wave = tid >> 6;
  const size_t nwaves = (static_cast<size_t>(gridDim.x) * blockDim.x) >> 6;
  const size_t nv = a.nv, len = a.nv * kN;
  const size_t resident = static_cast<size_t>(kKeep) << a.log2g;  // units the registers hold

  // wave-uniform bounds: every lane of the wave reaches the shuffles
  for (size_t first = wave * rows_per_wave; first < a.nrows; first += nwaves * rows_per_wave) {
    const RowAt at = Locate(a, first, lane);
    const bool lead = at.ok && gl == 0;
    const T* gp = grad + (at.live ? at.r * len : 0);
    uint16_t* tp = table + (at.ok ? at.row * len : 0);
    float* rec = state + (at.ok ? at.row * a.rec : 0);
    float* mp = rec + 4;
    float* vp = mp + len;  // element-wise only

    // the header first, then every resident unit of the row in one batch
    float4 h{1.f, 1.f, 0.f, 0.f};
    if (lead) h = LoadHeader<kVec>(rec);
    Held g[kKeep] = {};
    float m[kKeep][kN], v[kRowwise ? 1 : kKeep][kN];
    Packed w[kKeep] = {};
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < kKeep; ++k) {
      const size_t c = gl + (static_cast<size_t>(k) << a.log2g);
      if (at.ok && c < nv) {
        g[k] = W::Load(gp + c * kN);
        w[k] = U::LoadW(tp + c * kN);
        U::LoadF(mp + c * kN, m[k]);
        if (!kRowwise) U::LoadF(vp + c * kN, v[kRowwise ? 0 : k]);
      }
      if (kRowwise) ss += SumSqOf<W, kN>(g[k]);
    }
    if (kRowwise) {
      if (at.ok) {
        for (size_t c = resident + gl; c < nv; c += G) ss += SumSqOf<W, kN>(W::Load(gp + c * kN));
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

    if (!at.live) continue;  // past the shuffles: nothing below crosses lanes
    T* op = out ? out + at.r * len : nullptr;
    if (!at.ok) {
      if (out) ZeroRow<W, kN>(op, nv, gl, G);
      continue;
    }
    const uint64_t row_key = a.rd.stochastic ? RowKey(a.rd, at.row) : 0;
    auto apply = [&](size_t c, const Held& gh, Packed wv, float (&mv)[kN], float (&vv)[kN]) {
      float x[kN], gv[kN];
      W::Open(gh, gv);
      U::Unpack(wv, x);
#pragma unroll
      for (int j = 0; j < kN; ++j) {
        mv[j] = Moment(mv[j], gv[j], a.beta1, a.omb1);
        float denom = q;
        if (!kRowwise) {
          vv[j] = Moment(vv[j], gv[j] * gv[j], a.beta2, a.omb2);
          denom = AdamDenom(vv[j], q, a.eps);
        }
        x[j] = AdamStep(x[j], mv[j], alpha, denom);
      }
      U::StoreF(mp + c * kN, mv);
      if (!kRowwise) U::StoreF(vp + c * kN, vv);
      const Packed bits = Round<kN>(x, c, row_key, a.rd.stochastic);
      U::StoreW(tp + c * kN, bits);
      if (out) W::Store(op + c * kN, x, bits);
    };
#pragma unroll
    for (int k = 0; k < kKeep; ++k) {
      const size_t c = gl + (static_cast<size_t>(k) << a.log2g);
      if (c < nv) apply(c, g[k], w[k], m[k], v[kRowwise ? 0 : k]);
    }
    for (size_t c = resident + gl; c < nv; c += G) {
      float mv[kN], vv[kN];
      const Held gh = W::Load(gp + c * kN);
      U::LoadF(mp + c * kN, mv);
      if (!kRowwise) U::LoadF(vp + c * kN, vv);
      apply(c, gh, U::LoadW(tp + c * kN), mv, vv);
    }
  }
}

enum class Opt { kAdagrad, kLazyAdam };

template <Opt kOpt, int kN, bool kRowwise, class T>
void LaunchStepAs(uint16_t* table, float* state, const T* grad, T* out, StepArgs a, int grid_cap,
                  hipStream_t s) {
  while ((size_t{1} << a.log2g) < a.nv && a.log2g < 6) ++a.log2g;
  size_t rows_per_wave = 64 >> a.log2g;
  size_t waves = (a.nrows + rows_per_wave - 1) / rows_per_wave;
  // the sparse kernels' grid: enough blocks for the 8 XCDs, at most 16384
  int grid = GridFor(waves * 64, 16384, grid_cap);
  if (kOpt == Opt::kAdagrad) {
    hipLaunchKernelGGL((sparse_adagrad_bf16_kernel<kN, kRowwise, T>), dim3(grid), dim3(kBlock), 0,
                       s, table, state, grad, out, a);
  } else {
    hipLaunchKernelGGL((sparse_lazy_adam_bf16_kernel<kN, kRowwise, T>), dim3(grid), dim3(kBlock),
                       0, s, table, state, grad, out, a);
  }
}

template <Opt kOpt, class T>
void LaunchStep(uint16_t* table, float* state, const T* grad, T* out, size_t row_len, bool vec,
                bool rowwise, StepArgs a, int grid_cap, hipStream_t s) {
  a.nv = vec ? row_len / 8 : row_len;
  if (vec && rowwise) {
    LaunchStepAs<kOpt, 8, true>(table, state, grad, out, a, grid_cap, s);
  } else if (vec) {
    LaunchStepAs<kOpt, 8, false>(table, state, grad, out, a, grid_cap, s);
  } else if (rowwise) {
    LaunchStepAs<kOpt, 1, true>(table, state, grad, out, a, grid_cap, s);
  } else {
    LaunchStepAs<kOpt, 1, false>(table, state, grad, out, a, grid_cap, s);
  }
}

// what the steps share of a call; T is the wire's element
struct StepCall {
  const char* name;
  const uint64_t* rows;
  size_t nrows, row_len;
  bool rowwise;
  Bf16Rounding rounding;
  uint64_t seed;
  hipStream_t s;
  int key_shift;
  uint64_t row_base, table_rows;
  int grid_cap;
};
[[noreturn]] void Refuse(const StepCall& c, const char* what) {
  throw std::invalid_argument(std::string(c.name) + ": " + what);
}
StepArgs MakeStep(const StepCall& c, float lr, float eps) {
  StepArgs a{};
  a.rows = c.rows;
  a.nrows = c.nrows;
  a.row_len = static_cast<float>(c.row_len);
  a.lr = lr;
  a.eps = eps;
  a.shift = c.key_shift;
  a.base = c.row_base;
  a.tab_rows = c.table_rows;
  a.rd = Rounding{c.seed, c.rounding == Bf16Rounding::kStochastic};
  return a;
}

template <class T>
void Adagrad(uint16_t* table, float* state, const T* grad, T* out_or_null, float lr, float eps,
             const StepCall& c) {
  if (!(lr > 0.f)) Refuse(c, "lr must be positive");
  if (!(eps > 0.f)) Refuse(c, "eps must be positive");
  if (c.nrows == 0 || c.row_len == 0) return;
  // 8-element units need whole units and every array they move on a 16 B
  // boundary (the row-wise state moves as single floats)
  bool vec = c.row_len % 8 == 0 && Aligned16(table) && Aligned16(grad, out_or_null) &&
             (c.rowwise || Aligned16(state));
  LaunchStep<Opt::kAdagrad>(table, state, grad, out_or_null, c.row_len, vec, c.rowwise,
                            MakeStep(c, lr, eps), c.grid_cap, c.s);
}

template <class T>
void LazyAdam(uint16_t* table, float* state, const T* grad, T* out_or_null, float lr, float beta1,
              float beta2, float eps, const StepCall& c) {
  if (!(lr > 0.f)) Refuse(c, "lr must be positive");
  if (!(eps > 0.f)) Refuse(c, "eps must be positive");
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) {
    Refuse(c, "beta1 and beta2 must lie in [0, 1)");
  }
  // every record's header is one 16 B access on the vector path
  if (!Aligned16(state)) Refuse(c, "state must be 16 B-aligned");
  if (c.nrows == 0 || c.row_len == 0) return;
  StepArgs a = MakeStep(c, lr, eps);
  a.rec = SparseLazyAdamStateFloats(1, c.row_len, c.rowwise);
  a.beta1 = beta1;
  a.beta2 = beta2;
  a.omb1 = 1.f - beta1;
  a.omb2 = 1.f - beta2;
  // 8-element units need whole units and table, grad and out on a 16 B
  // boundary; the records' moments then are, their length being a multiple
  // of four floats
  bool vec = c.row_len % 8 == 0 && Aligned16(table) && Aligned16(grad, out_or_null);
  LaunchStep<Opt::kLazyAdam>(table, state, grad, out_or_null, c.row_len, vec, c.rowwise, a,
                             c.grid_cap, c.s);
}

template <class T>
void Gather(const uint16_t* table, const uint64_t* rows_dev, size_t nrows, size_t row_len, T* out,
            hipStream_t s, int key_shift, uint64_t row_base, uint64_t table_rows, int grid_cap) {
  MoveArgs a =
      MakeMove(rows_dev, nrows, key_shift, row_base, table_rows, Bf16Rounding::kNearest, 0);
  // the gather only reads the table
  LaunchMove<Move::kGather>(const_cast<uint16_t*>(table), out, row_len, a, grid_cap, s);
}

template <class T>
void Assign(uint16_t* table, const uint64_t* rows_dev, size_t nrows, size_t row_len, const T* src,
            hipStream_t s, int key_shift, uint64_t row_base, uint64_t table_rows, int grid_cap) {
  MoveArgs a =
      MakeMove(rows_dev, nrows, key_shift, row_base, table_rows, Bf16Rounding::kNearest, 0);
  // assign and add only read src
  LaunchMove<Move::kAssign>(table, const_cast<T*>(src), row_len, a, grid_cap, s);
}

template <class T>
void Add(uint16_t* table, const uint64_t* rows_dev, size_t nrows, size_t row_len, const T* src,
         Bf16Rounding rounding, uint64_t seed, hipStream_t s, int key_shift, uint64_t row_base,
         uint64_t table_rows, int grid_cap) {
  MoveArgs a = MakeMove(rows_dev, nrows, key_shift, row_base, table_rows, rounding, seed);
  LaunchMove<Move::kAdd>(table, const_cast<T*>(src), row_len, a, grid_cap, s);
}

}  // namespace

uint64_t SparseBf16LaunchSeed(uint64_t seed, uint64_t n) { return Mix64(seed + (n + 1) * kPhi); }

void SparseGatherBf16(const uint16_t* table, const uint64_t* rows_dev, size_t nrows,
                      size_t row_len, float* out, hipStream_t s, int key_shift, uint64_t row_base,
                      uint64_t table_rows, int grid_cap) {
  Gather(table, rows_dev, nrows, row_len, out, s, key_shift, row_base, table_rows, grid_cap);
}
void SparseGatherBf16Wire(const uint16_t* table, const uint64_t* rows_dev, size_t nrows,
                          size_t row_len, uint16_t* out, hipStream_t s, int key_shift,
                          uint64_t row_base, uint64_t table_rows, int grid_cap) {
  Gather(table, rows_dev, nrows, row_len, out, s, key_shift, row_base, table_rows, grid_cap);
}

void SparseScatterAssignBf16(uint16_t* table, const uint64_t* rows_dev, size_t nrows,
                             size_t row_len, const float* src, hipStream_t s, int key_shift,
                             uint64_t row_base, uint64_t table_rows, int grid_cap) {
  Assign(table, rows_dev, nrows, row_len, src, s, key_shift, row_base, table_rows, grid_cap);
}
void SparseScatterAssignBf16Wire(uint16_t* table, const uint64_t* rows_dev, size_t nrows,
                                 size_t row_len, const uint16_t* src, hipStream_t s, int key_shift,
                                 uint64_t row_base, uint64_t table_rows, int grid_cap) {
  Assign(table, rows_dev, nrows, row_len, src, s, key_shift, row_base, table_rows, grid_cap);
}

void SparseScatterAddBf16(uint16_t* table, const uint64_t* rows_dev, size_t nrows, size_t row_len,
                          const float* src, Bf16Rounding rounding, uint64_t seed, hipStream_t s,
                          int key_shift, uint64_t row_base, uint64_t table_rows, int grid_cap) {
  Add(table, rows_dev, nrows, row_len, src, rounding, seed, s, key_shift, row_base, table_rows,
      grid_cap);
}
void SparseScatterAddBf16Wire(uint16_t* table, const uint64_t* rows_dev, size_t nrows,
                              size_t row_len, const uint16_t* src, Bf16Rounding rounding,
                              uint64_t seed, hipStream_t s, int key_shift, uint64_t row_base,
                              uint64_t table_rows, int grid_cap) {
  Add(table, rows_dev, nrows, row_len, src, rounding, seed, s, key_shift, row_base, table_rows,
      grid_cap);
}

void SparseAdagradBf16(uint16_t* table, float* state, const uint64_t* rows_dev, size_t nrows,
                       size_t row_len, const float* grad, float* out_or_null, float lr, float eps,
                       bool rowwise, Bf16Rounding rounding, uint64_t seed, hipStream_t s,
                       int key_shift, uint64_t row_base, uint64_t table_rows, int grid_cap) {
  Adagrad(table, state, grad, out_or_null, lr, eps,
          StepCall{"SparseAdagradBf16", rows_dev, nrows, row_len, rowwise, rounding, seed, s,
                   key_shift, row_base, table_rows, grid_cap});
}
void SparseAdagradBf16Wire(uint16_t* table, float* state, const uint64_t* rows_dev, size_t nrows,
                           size_t row_len, const uint16_t* grad, uint16_t* out_or_null, float lr,
                           float eps, bool rowwise, Bf16Rounding rounding, uint64_t seed,
                           hipStream_t s, int key_shift, uint64_t row_base, uint64_t table_rows,
                           int grid_cap) {
  Adagrad(table, state, grad, out_or_null, lr, eps,
          StepCall{"SparseAdagradBf16Wire", rows_dev, nrows, row_len, rowwise, rounding, seed, s,
                   key_shift, row_base, table_rows, grid_cap});
}

void SparseLazyAdamBf16(uint16_t* table, float* state, const uint64_t* rows_dev, size_t nrows,
                        size_t row_len, const float* grad, float* out_or_null, float lr,
                        float beta1, float beta2, float eps, bool rowwise, Bf16Rounding rounding,
                        uint64_t seed, hipStream_t s, int key_shift, uint64_t row_base,
                        uint64_t table_rows, int grid_cap) {
  LazyAdam(table, state, grad, out_or_null, lr, beta1, beta2, eps,
           StepCall{"SparseLazyAdamBf16", rows_dev, nrows, row_len, rowwise, rounding, seed, s,
                    key_shift, row_base, table_rows, grid_cap});
}
void SparseLazyAdamBf16Wire(uint16_t* table, float* state, const uint64_t* rows_dev, size_t nrows,
                            size_t row_len, const uint16_t* grad, uint16_t* out_or_null, float lr,
                            float beta1, float beta2, float eps, bool rowwise,
                            Bf16Rounding rounding, uint64_t seed, hipStream_t s, int key_shift,
                            uint64_t row_base, uint64_t table_rows, int grid_cap) {
  LazyAdam(table, state, grad, out_or_null, lr, beta1, beta2, eps,
           StepCall{"SparseLazyAdamBf16Wire", rows_dev, nrows, row_len, rowwise, rounding, seed, s,
                    key_shift, row_base, table_rows, grid_cap});
}

}  // namespace kern
}  // namespace xps
