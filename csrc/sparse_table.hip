// The sparse handler's kernels over an embedding table for CDNA4 (gfx950):
// the five entry points of kernels.h (gather, assign, add, and the Adagrad
// and lazy-Adam steps), the optimizer steps for every table, and the moves of
// a bf16 table (the fp32 table's moves are kernels.hip's). A step updates the
// pushed rows and optionally writes the post-update rows to a second
// destination in the same pass (the fused ZPushPull round: no gather launch,
// no second read of the table).
//
// A table stores fp32 values or bf16 bits; the optimizer state is fp32 either
// way. A step widens a bf16 weight exactly, runs sparse_elem.h's fp32
// arithmetic, the same for every table, and rounds once on the store. The
// wire side (the gradients and pushed values, the returned rows) is fp32 or,
// for a bf16 table, bf16 bits: a 16-bit gradient is widened exactly and a
// 16-bit row out is the stored bits, so the two wires leave the same table
// and state bits for the same values.
//
// The store rule R(x) of a bf16 table, u the bits of x: nearest is
// round-to-nearest-even; stochastic stores (u + r) >> 16 with r uniform in
// [0, 2^16), so the magnitude goes up with probability (u & 0xffff) / 2^16
// and a value that already is a bf16 keeps its bits whatever r is. Inf and
// NaN pass through both (a NaN keeps a mantissa bit). r is a field of a
// counter-based 64-bit word: SplitMix64 seeded per row,
//   row_key = mix(seed + (row + 1) * phi)          row = the local table row
//   word(q) = mix(row_key + (q + 1) * phi)         q = element index / 4
//   r       = (word >> 16 * (element index % 4)) & 0xffff
// phi = 0x9E3779B97F4A7C15 and mix the SplitMix64 finalizer. No state, no
// dependence on lanes, waves or the grid: the same call gives the same bits
// on the vector and the scalar path and under any grid_cap. An fp32 table's
// R is the identity.
//
// Work split of the steps, wave64, no LDS: one body (sparse_step_kernel) for
// every table, wire and optimizer but the fp32 table's Adagrad, which keeps a
// narrower one on the same pieces (sparse_adagrad_f32_kernel, and why). A
// lane's unit is kUnit elements of every
// array of a row, kUnit the table's: 8 for a bf16 table (one 16 B access of
// the table against two float4 each of gradient, moments and out, or one
// 16 B access of a 16-bit gradient and out), 4 for an fp32 table (one float4
// of each). A row belongs to a group of G lanes, G the smallest power of two
// >= row_len / kUnit, at most 64; a wave serves 64 / G rows per pass and
// waves take sets of rows in a grid-stride loop. The loop bound is the same
// for every lane of a wave, so lanes without a row or without a column (a
// short last set, a row whose unit count is no power of two, a key outside
// the table) stay in the loop, give zero to the cross-lane sum and reach the
// shuffles. The group's first lane loads the row's own state (the row-wise
// Adagrad sum, the lazy-Adam header) before anything else, so its latency
// hides behind the row's loads; every lane loads its kKeep resident units of
// gradient, weight and element-wise state in one batch ahead of the
// cross-lane sum (bf16 weights and 16-bit gradients stay packed, 4 registers
// per unit), so the update that follows the shuffles waits for no memory.
// kKeep is the table's, 16 resident elements per lane either way: 2 units of
// a bf16 table, 4 of an fp32 table. The first lane forms the row's scalars
// and stores the row's state once, and shuffles hand the scalars to the
// group. Rows past kKeep * 64 * kUnit = 1024 elements stream the rest
// through the update from memory, the gradient read a second time. The
// scalar path (row_len % kUnit != 0 or a pointer off its 16 B boundary) is
// the same body with a unit of one element for the whole call.
//
// A row's lazy-Adam state is one record,
//   { p1, p2, v_row, 0 }  m[row_len]  v[row_len] (element-wise only)
// p1 and p2 the running products beta1^t and beta2^t of the row's own steps
// (1 before the first), so a random row costs one DRAM region, not three.
// The header moves as one 16 B load and one 16 B store on the vector paths.
//
// Traffic per row of L elements, by construction: row-wise Adagrad with out
// 16 L bytes (bf16 table: 12 L; with a 16-bit wire: 8 L), row-wise lazy Adam
// 24 L + 32 (20 L + 32; 16 L + 32), element-wise lazy Adam 8 L more, gather
// 8 L (6 L; 4 L).
//
// Lazy Adam: the exact order of the fp32 operations, one IEEE rounding each.
// The moments' multiply-adds are compiled uncontracted (sparse_elem.h); the
// one product left next to a subtraction is p' in 1 - p', where the compiler
// may use the unrounded p * beta (the tests' bound allows for both).
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
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <type_traits>

#include "kernels.h"
#include "sparse_move_f32.h"
#include "sparse_elem.h"

namespace xps {
namespace kern {

namespace {

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

// kN floats of an fp32 array (a gradient, a moment, a row out): float4
// accesses for a vector unit, one float for the scalar unit
template <int kN>
__device__ inline void LoadF(const float* p, float (&x)[kN]) {
  if constexpr (kN == 1) {
    x[0] = *p;
  } else {
#pragma unroll
    for (int i = 0; i < kN; i += 4) {
      const float4 v = *reinterpret_cast<const float4*>(p + i);
      x[i] = v.x, x[i + 1] = v.y, x[i + 2] = v.z, x[i + 3] = v.w;
    }
  }
}
template <int kN>
__device__ inline void StoreF(float* p, const float (&x)[kN]) {
  if constexpr (kN == 1) {
    *p = x[0];
  } else {
#pragma unroll
    for (int i = 0; i < kN; i += 4) {
      *reinterpret_cast<float4*>(p + i) = float4{x[i], x[i + 1], x[i + 2], x[i + 3]};
    }
  }
}

// A unit of kN elements as an array holds it: T the array's element, Packed
// what a lane keeps of a loaded unit, Unpack its fp32 values.
template <int kN>
struct F32Unit {
  using T = float;
  struct Packed {
    float x[kN];
  };
  static __device__ inline Packed Load(const float* p) {
    Packed v;
    LoadF(p, v.x);
    return v;
  }
  static __device__ inline void Store(float* p, const Packed& v) { StoreF(p, v.x); }
  static __device__ inline void Unpack(const Packed& v, float (&x)[kN]) {
#pragma unroll
    for (int j = 0; j < kN; ++j) x[j] = v.x[j];
  }
};
template <int kN>
struct Bf16Unit;
template <>
struct Bf16Unit<8> {
  using T = uint16_t;
  using Packed = uint4;
  static __device__ inline uint4 Load(const uint16_t* p) {
    return *reinterpret_cast<const uint4*>(p);
  }
  static __device__ inline void Store(uint16_t* p, uint4 v) { *reinterpret_cast<uint4*>(p) = v; }
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
};
template <>
struct Bf16Unit<1> {
  using T = uint16_t;
  using Packed = uint16_t;
  static __device__ inline uint16_t Load(const uint16_t* p) { return *p; }
  static __device__ inline void Store(uint16_t* p, uint16_t v) { *p = v; }
  static __device__ inline void Unpack(uint16_t p, float (&x)[1]) { x[0] = Widen(p); }
  static __device__ inline uint16_t Pack(const uint16_t (&b)[1]) { return b[0]; }
};

// The table side of a unit. kUnit: the elements of a vector unit; kKeep: the
// resident units of a lane, 16 elements of each array either way. Round is R
// over unit c of a row: the packed form to store, x left as what a later
// gather returns. RowKey is what R needs of the row.
template <int kN>
struct F32Table : F32Unit<kN> {
  static constexpr int kUnit = 4, kKeep = 4;
  static __device__ inline uint64_t RowKey(const Rounding&, uint64_t) { return 0; }
  static __device__ inline typename F32Unit<kN>::Packed Round(float (&x)[kN], size_t, uint64_t,
                                                              bool) {
    typename F32Unit<kN>::Packed v;
#pragma unroll
    for (int j = 0; j < kN; ++j) v.x[j] = x[j];
    return v;
  }
};
// kKeep = 4 was measured for the 16-bit wire's smaller gradient unit
// (profiles/sparse_bf16_wire.md): faster at row length 2048, slower at 64 on
// both wires, so it stays 2.
template <int kN>
struct Bf16Table : Bf16Unit<kN> {
  static constexpr int kUnit = 8, kKeep = 2;
  static __device__ inline uint64_t RowKey(const Rounding& rd, uint64_t row) {
    return rd.stochastic ? Mix64(rd.seed + (row + 1) * kPhi) : 0;
  }
  // x left as the stored bits widened
  static __device__ inline typename Bf16Unit<kN>::Packed Round(float (&x)[kN], size_t c,
                                                               uint64_t row_key, bool stochastic) {
    uint16_t b[kN];
    uint64_t word = 0;
#pragma unroll
    for (int j = 0; j < kN; ++j) {
      const size_t e = c * kN + j;  // the element's index in its row
      if (stochastic && (kN == 1 || j % 4 == 0)) word = Mix64(row_key + ((e >> 2) + 1) * kPhi);
      b[j] = RoundBf16(x[j], static_cast<uint32_t>(word >> (16 * (e & 3))) & 0xffffu, stochastic);
      x[j] = Widen(b[j]);
    }
    return Bf16Unit<kN>::Pack(b);
  }
};
template <class T, int kN>
using TableOf = std::conditional_t<std::is_same<T, float>::value, F32Table<kN>, Bf16Table<kN>>;

// The wire side of a unit: the gradient or pushed values in, the rows out.
// Put writes a unit of rows out, given both its values x and the table's
// stored form of them: an fp32 wire takes the values, a 16-bit wire the bits.
template <int kN>
struct F32Wire : F32Unit<kN> {
  template <class Stored>
  static __device__ inline void Put(float* p, const float (&x)[kN], const Stored&) {
    StoreF(p, x);
  }
};
template <int kN>
struct Bf16Wire : Bf16Unit<kN> {
  static __device__ inline void Put(uint16_t* p, const float (&)[kN],
                                    typename Bf16Unit<kN>::Packed bits) {
    Bf16Unit<kN>::Store(p, bits);
  }
};
template <class T, int kN>
using WireOf = std::conditional_t<std::is_same<T, float>::value, F32Wire<kN>, Bf16Wire<kN>>;

template <int kN>
__device__ inline void Zero(float (&x)[kN]) {
#pragma unroll
  for (int j = 0; j < kN; ++j) x[j] = 0.f;
}

// what a move kernel knows of its call
struct RowArgs {
  const uint64_t* rows;
  size_t nrows;
  size_t nv;  // units per row
  int shift;
  uint64_t base;
  uint64_t tab_rows;
  Rounding rd;
};
RowArgs MakeRows(const SparseRows& r, const SparseTable& t, bool rounds) {
  RowArgs a{};
  a.rows = r.keys;
  a.nrows = r.nrows;
  a.shift = r.key_shift;
  a.base = r.row_base;
  a.tab_rows = r.table_rows;
  a.rd = Rounding{t.seed, rounds && t.rounding == Bf16Rounding::kStochastic};
  return a;
}

// ----------------------------------- gather, assign, add of a bf16 table

enum class Move { kGather, kAssign, kAdd };

// one unit of one message row per lane and step, grid-stride; f is the wire
// side: out (gather), src (assign, add). A 16-bit gather and assign move
// bits: the worker rounded what it assigns.
template <int kN, Move kOp, class T>
__global__ void __launch_bounds__(kBlock)
    sparse_move_bf16_kernel(uint16_t* __restrict__ table, T* __restrict__ f, RowArgs a) {
  using U = Bf16Table<kN>;
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
        W::Put(f + i * kN, x, Packed{});
      }
      continue;
    }
    uint16_t* tp = table + (row * a.nv + c) * kN;
    if (kOp == Move::kGather) {
      const Packed p = U::Load(tp);
      U::Unpack(p, x);
      W::Put(f + i * kN, x, p);
      continue;
    }
    const typename W::Packed h = W::Load(f + i * kN);
    if constexpr (kOp == Move::kAssign && std::is_same<T, uint16_t>::value) {
      U::Store(tp, h);
      continue;
    }
    W::Unpack(h, x);
    if (kOp == Move::kAdd) {
      float w[kN];
      U::Unpack(U::Load(tp), w);
#pragma unroll
      for (int j = 0; j < kN; ++j) x[j] = w[j] + x[j];
    }
    const bool stochastic = kOp == Move::kAdd && a.rd.stochastic;
    U::Store(tp, U::Round(x, c, U::RowKey(a.rd, row), stochastic));
  }
}

// f is only read by assign and add, the table only by gather
template <Move kOp, class T>
void LaunchMove(uint16_t* table, T* f, const SparseRows& r, RowArgs a) {
  if (r.nrows == 0 || r.row_len == 0) return;
  const bool vec = r.row_len % 8 == 0 && Aligned16(table) && Aligned16(f);
  a.nv = vec ? r.row_len / 8 : r.row_len;
  int grid = GridFor(a.nrows * a.nv, 16384, r.grid_cap);
  if (vec) {
    hipLaunchKernelGGL((sparse_move_bf16_kernel<8, kOp, T>), dim3(grid), dim3(kBlock), 0, r.s,
                       table, f, a);
  } else {
    hipLaunchKernelGGL((sparse_move_bf16_kernel<1, kOp, T>), dim3(grid), dim3(kBlock), 0, r.s,
                       table, f, a);
  }
}

// ------------------------------------------------------ optimizer steps

// What a step kernel knows of its call. The order is part of the kernel: a
// wave's first scalar loads take rows .. rec and log2g, and with the fields in
// this order they touch every 64 B line of the arguments at once; with the
// row fields gathered in a leading RowArgs a line was left to a second round
// trip, 0.2 us on every launch.
struct StepArgs {
  const uint64_t* rows;
  size_t nrows;
  size_t nv;      // units per row
  size_t rec;     // floats of a row's state record
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

// An optimizer, as the step body sees it. A row's state is a record of
// a.rec floats: kHeader floats of the row's own, which the group's first lane
// moves (Row, LoadRow), then kArrays arrays of row_len floats, which move like
// the table. kSumSq: Lead wants the row's sum of g * g. Lead, the first lane
// alone: the record's header forward and stored, the row's kScalars scalars
// into sc. Elem: one element's update under those scalars, s0 and s1 its
// values in the arrays.
constexpr int kMaxArrays = 2, kMaxScalars = 2;

template <bool kRowwise>
struct AdagradOpt {
  static constexpr bool kSumSq = kRowwise;
  static constexpr int kHeader = kRowwise ? 1 : 0, kArrays = kRowwise ? 0 : 1;
  static constexpr int kScalars = kRowwise ? 1 : 0;  // the row's denominator
  static constexpr bool kOwnF32Body = true;  // sparse_adagrad_f32_kernel, below
  struct Row {};  // the row's sum is read where it is advanced
  template <bool kVec>
  static __device__ inline Row LoadRow(const float*) {
    return Row{};
  }
  template <bool kVec>
  static __device__ inline void Lead(float* rec, Row, float ss, const StepArgs& a,
                                     float (&sc)[kMaxScalars]) {
    const float s = *rec + ss / a.row_len;
    *rec = s;
    sc[0] = Denom(s, a.eps);
  }
  static __device__ inline void Elem(float& x, float g, float& s, float&,
                                     const float (&sc)[kMaxScalars], const StepArgs& a) {
    if (kRowwise) {
      x = Step(x, g, a.lr, sc[0]);
    } else {
      s += g * g;
      x = Step(x, g, a.lr, Denom(s, a.eps));
    }
  }
};

template <bool kRowwise>
struct LazyAdamOpt {
  static constexpr bool kSumSq = kRowwise;
  static constexpr int kHeader = 4, kArrays = kRowwise ? 1 : 2;
  static constexpr int kScalars = 2;  // alpha, and q = the denominator (row-wise) or c2
  static constexpr bool kOwnF32Body = false;
  using Row = float4;
  template <bool kVec>
  static __device__ inline float4 LoadRow(const float* rec) {
    return LoadHeader<kVec>(rec);
  }
  template <bool kVec>
  static __device__ inline void Lead(float* rec, float4 h, float ss, const StepArgs& a,
                                     float (&sc)[kMaxScalars]) {
    h.x = h.x * a.beta1;
    h.y = h.y * a.beta2;
    sc[0] = a.lr / (1.f - h.x);
    sc[1] = 1.f - h.y;
    if (kRowwise) {
      h.z = Moment(h.z, ss / a.row_len, a.beta2, a.omb2);
      sc[1] = AdamDenom(h.z, sc[1], a.eps);
    }
    StoreHeader<kVec>(rec, h);
  }
  static __device__ inline void Elem(float& x, float g, float& m, float& v,
                                     const float (&sc)[kMaxScalars], const StepArgs& a) {
    m = Moment(m, g, a.beta1, a.omb1);
    float denom = sc[1];
    if (!kRowwise) {
      v = Moment(v, g * g, a.beta2, a.omb2);
      denom = AdamDenom(v, sc[1], a.eps);
    }
    x = AdamStep(x, m, sc[0], denom);
  }
};

template <class W, int kN>
__device__ inline float SumSq(const typename W::Packed& h) {
  float g[kN];
  W::Unpack(h, g);
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < kN; ++j) ss += g[j] * g[j];
  return ss;
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
template <class Tab, class W, int kN>
__device__ inline void ZeroRow(typename W::T* out, size_t nv, int gl, int G) {
  float z[kN];
  Zero(z);
  for (size_t c = gl; c < nv; c += G) W::Put(out + c * kN, z, typename Tab::Packed{});
}

template <int kN, class TT, class WT, class Opt>
__global__ void __launch_bounds__(kBlock)
    sparse_step_kernel(TT* __restrict__ table, float* __restrict__ state,
                       const WT* __restrict__ grad, WT* __restrict__ out, StepArgs a) {
  using Tab = TableOf<TT, kN>;
  using W = WireOf<WT, kN>;
  using Stored = typename Tab::Packed;
  using Held = typename W::Packed;
  constexpr int kKeep = Tab::kKeep;
  constexpr bool kVec = kN > 1;
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
    const WT* gp = grad + (at.live ? at.r * len : 0);
    TT* tp = table + (at.ok ? at.row * len : 0);
    float* rec = state + (at.ok ? at.row * a.rec : 0);
    float* sp[kMaxArrays];  // the record's arrays
#pragma unroll
    for (int i = 0; i < kMaxArrays; ++i) sp[i] = rec + Opt::kHeader + i * len;

    // the row's own state first, then every resident unit of the row in one batch
    typename Opt::Row h{};
    if (Opt::kHeader && lead) h = Opt::template LoadRow<kVec>(rec);
    Held g[kKeep] = {};
    Stored w[kKeep] = {};
    float st[kMaxArrays][kKeep][kN];
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < kKeep; ++k) {
      const size_t c = gl + (static_cast<size_t>(k) << a.log2g);
      if (at.ok && c < nv) {
        g[k] = W::Load(gp + c * kN);
        w[k] = Tab::Load(tp + c * kN);
#pragma unroll
        for (int i = 0; i < Opt::kArrays; ++i) LoadF(sp[i] + c * kN, st[i][k]);
      }
      if (Opt::kSumSq) ss += SumSq<W, kN>(g[k]);
    }
    if (Opt::kSumSq) {
      if (at.ok) {
        for (size_t c = resident + gl; c < nv; c += G) ss += SumSq<W, kN>(W::Load(gp + c * kN));
      }
      for (int m = G >> 1; m > 0; m >>= 1) ss += __shfl_xor(ss, m);
    }

    // the row's scalars, from its first lane
    float sc[kMaxScalars] = {};
    if (Opt::kHeader && lead) Opt::template Lead<kVec>(rec, h, ss, a, sc);
#pragma unroll
    for (int i = 0; i < Opt::kScalars; ++i) sc[i] = __shfl(sc[i], lane - gl);

    if (!at.live) continue;  // past the shuffles: nothing below crosses lanes
    WT* op = out ? out + at.r * len : nullptr;
    if (!at.ok) {
      if (out) ZeroRow<Tab, W, kN>(op, nv, gl, G);
      continue;
    }
    const uint64_t row_key = Tab::RowKey(a.rd, at.row);
    auto apply = [&](size_t c, const Held& gh, const Stored& wv, float (&s0)[kN],
                     float (&s1)[kN]) {
      float x[kN], gv[kN];
      W::Unpack(gh, gv);
      Tab::Unpack(wv, x);
#pragma unroll
      for (int j = 0; j < kN; ++j) Opt::Elem(x[j], gv[j], s0[j], s1[j], sc, a);
      if (Opt::kArrays > 0) StoreF(sp[0] + c * kN, s0);
      if (Opt::kArrays > 1) StoreF(sp[1] + c * kN, s1);
      const Stored bits = Tab::Round(x, c, row_key, a.rd.stochastic);
      Tab::Store(tp + c * kN, bits);
      if (out) W::Put(op + c * kN, x, bits);
    };
#pragma unroll
    for (int k = 0; k < kKeep; ++k) {
      const size_t c = gl + (static_cast<size_t>(k) << a.log2g);
      if (c < nv) apply(c, g[k], w[k], st[0][k], st[1][k]);
    }
    for (size_t c = resident + gl; c < nv; c += G) {
      float sv[kMaxArrays][kN];
      const Held gh = W::Load(gp + c * kN);
#pragma unroll
      for (int i = 0; i < Opt::kArrays; ++i) LoadF(sp[i] + c * kN, sv[i]);
      apply(c, gh, Tab::Load(tp + c * kN), sv[0], sv[1]);
    }
  }
}

// The fp32 table's Adagrad step keeps a body of its own, on StepArgs, Locate
// and the shared launch geometry and checks: only the gradient is resident,
// and weights and state are read in the update, which holds the float4
// kernels at 64 (element-wise: 71) VGPRs and 8 (7) waves per SIMD. In the
// body above they take 82 (91) VGPRs and 5 waves. It sits on that edge: its
// rows move as V, not as float[kN], and ZeroRow in place of its zero loop
// already costs the row-wise kernel a wave (71 VGPRs).
__device__ inline float SumSqV(float v) { return v * v; }
__device__ inline float SumSqV(float4 v) { return v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w; }

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

template <class V, bool kRowwise>
__global__ void __launch_bounds__(kBlock)
    sparse_adagrad_f32_kernel(V* __restrict__ table, float* __restrict__ state,
                              const V* __restrict__ grad, V* __restrict__ out, StepArgs a) {
  const int G = 1 << a.log2g;
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1);  // lane within the row's group
  const size_t rows_per_wave = 64 >> a.log2g;
  const size_t tid = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  const size_t wave = tid >> 6;
  const size_t nwaves = (static_cast<size_t>(gridDim.x) * blockDim.x) >> 6;
  const size_t nv = a.nv;
  constexpr int kKeep = F32Table<1>::kKeep;
  const size_t resident = static_cast<size_t>(kKeep) << a.log2g;  // vectors the registers hold
  const V zero{};

  // wave-uniform bounds: every lane of the wave reaches the shuffles
  for (size_t first = wave * rows_per_wave; first < a.nrows; first += nwaves * rows_per_wave) {
    const RowAt at = Locate(a, first, lane);
    const size_t r = at.r;
    const uint64_t row = at.row;
    const bool live = at.live, ok = at.ok;
    const V* gp = grad + (live ? r * nv : 0);
    V* tp = table + (ok ? row * nv : 0);

    V g[kKeep];
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < kKeep; ++k) {
      const size_t c = gl + (static_cast<size_t>(k) << a.log2g);
      g[k] = (ok && c < nv) ? gp[c] : zero;
      if (kRowwise) ss += SumSqV(g[k]);
    }

    float denom = 0.f;
    if (kRowwise) {
      if (ok) {
        for (size_t c = resident + gl; c < nv; c += G) ss += SumSqV(gp[c]);
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

// the lane groups and the grid of a step over a.nv units per row
template <int kN, class Opt, class TT, class WT>
void LaunchStepAs(TT* table, float* state, const WT* grad, WT* out, StepArgs a,
                  const SparseRows& r) {
  while ((size_t{1} << a.log2g) < a.nv && a.log2g < 6) ++a.log2g;
  size_t rows_per_wave = 64 >> a.log2g;
  size_t waves = (a.nrows + rows_per_wave - 1) / rows_per_wave;
  // the sparse kernels' grid: enough blocks for the 8 XCDs, at most 16384
  int grid = GridFor(waves * 64, 16384, r.grid_cap);
  if constexpr (Opt::kOwnF32Body && std::is_same<TT, float>::value) {
    using V = std::conditional_t<kN == 1, float, float4>;
    hipLaunchKernelGGL((sparse_adagrad_f32_kernel<V, Opt::kSumSq>), dim3(grid), dim3(kBlock), 0,
                       r.s, reinterpret_cast<V*>(table), state, reinterpret_cast<const V*>(grad),
                       reinterpret_cast<V*>(out), a);
  } else {
    hipLaunchKernelGGL((sparse_step_kernel<kN, TT, WT, Opt>), dim3(grid), dim3(kBlock), 0, r.s,
                       table, state, grad, out, a);
  }
}

// Vector units need whole units and every array they move on a 16 B boundary:
// table, grad, out, and a state whose arrays start at its base (element-wise
// Adagrad; the row-wise state moves as single floats, and lazy Adam's records
// are aligned by the caller's check, their length a multiple of four floats).
template <template <bool> class Opt, class TT, class WT>
void LaunchStep(TT* table, float* state, const WT* grad, WT* out, bool rowwise, StepArgs a,
                const SparseRows& r) {
  constexpr int kUnit = TableOf<TT, 1>::kUnit;
  const bool vec = r.row_len % kUnit == 0 && Aligned16(table) && Aligned16(grad, out) &&
                   (rowwise || Aligned16(state));
  a.nv = vec ? r.row_len / kUnit : r.row_len;
  if (vec && rowwise) {
    LaunchStepAs<kUnit, Opt<true>>(table, state, grad, out, a, r);
  } else if (vec) {
    LaunchStepAs<kUnit, Opt<false>>(table, state, grad, out, a, r);
  } else if (rowwise) {
    LaunchStepAs<1, Opt<true>>(table, state, grad, out, a, r);
  } else {
    LaunchStepAs<1, Opt<false>>(table, state, grad, out, a, r);
  }
}

// ---------------------------------------------------- the entry points

[[noreturn]] void Refuse(const char* name, const char* what) {
  throw std::invalid_argument(std::string(name) + ": " + what);
}

// fn(table, wire) with the pointers typed by the call's dtypes; the pairs
// without a kernel are refused
template <class Fn>
void WithTypes(const char* name, const SparseTable& t, const SparseWire& w, Fn fn) {
  if (t.dtype == SparseDtype::kF32 && w.dtype == SparseDtype::kF32) {
    fn(static_cast<float*>(t.p), static_cast<float*>(w.p));
  } else if (t.dtype == SparseDtype::kF32) {
    Refuse(name, "an fp32 table has no bf16 wire");
  } else if (w.dtype == SparseDtype::kF32) {
    fn(static_cast<uint16_t*>(t.p), static_cast<float*>(w.p));
  } else {
    fn(static_cast<uint16_t*>(t.p), static_cast<uint16_t*>(w.p));
  }
}

template <template <bool> class Opt>
void RunStep(const char* name, const SparseTable& t, float* state, const SparseRows& r,
             const SparseWire& grad, const SparseWire& out, bool rowwise,
             const StepArgs& params) {
  if (out.p && out.dtype != grad.dtype) Refuse(name, "grad and out must be of one dtype");
  WithTypes(name, t, grad, [&](auto* table, auto* g) {
    if (r.nrows == 0 || r.row_len == 0) return;
    StepArgs a = params;
    const RowArgs rows = MakeRows(r, t, /*rounds=*/true);
    a.rows = rows.rows;
    a.nrows = rows.nrows;
    a.shift = rows.shift;
    a.base = rows.base;
    a.tab_rows = rows.tab_rows;
    a.rd = rows.rd;
    a.row_len = static_cast<float>(r.row_len);
    LaunchStep<Opt>(table, state, g, static_cast<decltype(g)>(out.p), rowwise, a, r);
  });
}

void CheckStep(const char* name, float lr, float eps) {
  if (!(lr > 0.f)) Refuse(name, "lr must be positive");
  if (!(eps > 0.f)) Refuse(name, "eps must be positive");
}

}  // namespace

uint64_t SparseBf16LaunchSeed(uint64_t seed, uint64_t n) { return Mix64(seed + (n + 1) * kPhi); }

size_t SparseLazyAdamStateFloats(size_t rows, size_t row_len, bool rowwise) {
  return rows * (4 + row_len * (rowwise ? 1 : 2));
}

void SparseGather(const SparseTable& t, const SparseRows& r, SparseWire out) {
  WithTypes("SparseGather", t, out, [&](auto* table, auto* f) {
    if constexpr (std::is_same<decltype(table), float*>::value) {
      SparseGatherF32(table, r, f);
    } else {
      LaunchMove<Move::kGather>(table, f, r, MakeRows(r, t, /*rounds=*/false));
    }
  });
}

void SparseScatterAssign(const SparseTable& t, const SparseRows& r, SparseWire src) {
  WithTypes("SparseScatterAssign", t, src, [&](auto* table, auto* f) {
    if constexpr (std::is_same<decltype(table), float*>::value) {
      SparseScatterAssignF32(table, r, f);
    } else {
      LaunchMove<Move::kAssign>(table, f, r, MakeRows(r, t, /*rounds=*/false));
    }
  });
}

void SparseScatterAdd(const SparseTable& t, const SparseRows& r, SparseWire src, bool atomic) {
  if (atomic && t.dtype != SparseDtype::kF32) {
    Refuse("SparseScatterAdd", "a bf16 table has no atomic add");
  }
  WithTypes("SparseScatterAdd", t, src, [&](auto* table, auto* f) {
    if constexpr (std::is_same<decltype(table), float*>::value) {
      SparseScatterAddF32(table, r, f, atomic);
    } else {
      LaunchMove<Move::kAdd>(table, f, r, MakeRows(r, t, /*rounds=*/true));
    }
  });
}

void SparseAdagrad(const SparseTable& t, float* state, const SparseRows& r, SparseWire grad,
                   SparseWire out_or_null, const AdagradParams& p) {
  CheckStep("SparseAdagrad", p.lr, p.eps);
  StepArgs a{};
  a.rec = p.rowwise ? 1 : r.row_len;
  a.lr = p.lr;
  a.eps = p.eps;
  RunStep<AdagradOpt>("SparseAdagrad", t, state, r, grad, out_or_null, p.rowwise, a);
}

void SparseLazyAdam(const SparseTable& t, float* state, const SparseRows& r, SparseWire grad,
                    SparseWire out_or_null, const LazyAdamParams& p) {
  CheckStep("SparseLazyAdam", p.lr, p.eps);
  if (!(p.beta1 >= 0.f && p.beta1 < 1.f) || !(p.beta2 >= 0.f && p.beta2 < 1.f)) {
    Refuse("SparseLazyAdam", "beta1 and beta2 must lie in [0, 1)");
  }
  // every record's header is one 16 B access on the vector paths
  if (!Aligned16(state)) Refuse("SparseLazyAdam", "state must be 16 B-aligned");
  StepArgs a{};
  a.rec = SparseLazyAdamStateFloats(1, r.row_len, p.rowwise);
  a.lr = p.lr;
  a.beta1 = p.beta1;
  a.beta2 = p.beta2;
  a.omb1 = 1.f - p.beta1;
  a.omb2 = 1.f - p.beta2;
  a.eps = p.eps;
  RunStep<LazyAdamOpt>("SparseLazyAdam", t, state, r, grad, out_or_null, p.rowwise, a);
}

}  // namespace kern
}  // namespace xps
