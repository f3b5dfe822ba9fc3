// Worker-side coalescing of a sparse message for CDNA4 (gfx950): from the
// ids of a batch (any order, any repetition) and one gradient row per
// occurrence to the sorted unique keys, one summed row per key and, for
// every occurrence, the slot of its key. The sums add a key's rows in
// ascending occurrence index, one IEEE fp32 add each, so the message is a
// function of the inputs alone. The sums leave as fp32, or for a 16-bit wire
// as bf16 bits: the same fp32 sum, rounded once to nearest even on the store.
//
// Tile size: kTile = 1024 elements, 4 per lane of a 256-lane block; key and
// occurrence index sit in LDS as two arrays (8 B + 4 B per element), 12 KB
// per block. Measured at 512, 1024, 2048 and 4096 (profiles/
// sparse_coalesce.md): the bitonic network in LDS (55 barrier steps at
// 1024, 66 at 2048, 78 at 4096) costs more than the merge pass a larger
// tile saves, and from 2048 on LDS holds the kernels below 8 waves per
// SIMD, so 2048 and 4096 lose at every size timed. 512 is 7-23 us ahead
// of 1024 from 2048 ids up but pays four more launches for 513..1024 ids
// (72-75 us against 60-62); 1024 keeps such messages on the two-launch
// path.
//
// Launches, all wave64, none waits on another block:
//   n <= kTile: coalesce_small (sort, heads, scan and emit of the one
//               tile), then coalesce_row_sums.
//   otherwise:  coalesce_tile_sort     one sorted run per tile
//               coalesce_merge         x ceil(log2(tiles)), ping-pong
//               coalesce_count_heads   heads per tile
//               coalesce_scan_tiles    one block: exclusive scan, m
//               coalesce_emit          keys, inverse, segment starts
//               coalesce_row_sums
// The order is the lexicographic one on (key, occurrence index), which is
// total: the sorted permutation is unique, equal keys lie in ascending
// index, and the padding (max key, max index) of a short tile sorts behind
// a real all-ones key because a real index is below 2^31.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "kernels.h"

namespace xps {
namespace kern {

namespace {

constexpr uint32_t kTile = 1024;
constexpr uint32_t kItems = kTile / kBlock;  // elements a lane merges and emits
constexpr int kAhead = 8;                    // occurrences whose rows are loaded before the adds
constexpr uint32_t kNone = 0xFFFFFFFFu;
static_assert(kTile % kBlock == 0 && (kTile & (kTile - 1)) == 0, "tile: a power of two of lanes");
static_assert(kTile * 12 <= 64 * 1024, "tile: key and index within 64 KB of LDS");

__device__ inline bool Less(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
  return ka < kb || (ka == kb && ia < ib);
}

// Exclusive scan of v over the block's 256 lanes; *total = the block's sum.
// Every lane calls it; wsum holds one word per wave.
__device__ inline uint32_t BlockScan(uint32_t v, uint32_t* wsum, uint32_t* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    uint32_t up = __shfl_up(inc, d);
    if (lane >= d) inc += up;
  }
  __syncthreads();  // wsum may still be read from the call before
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (int k = 0; k < kBlock / 64; ++k) {
    uint32_t t = wsum[k];
    if (k < w) before += t;
    all += t;
  }
  *total = all;
  return before + inc - v;
}

// Loads ids[base, base + count) with their indices into LDS, pads to the
// next power of two S and sorts [0, S) by (key, index), ascending.
__device__ inline void TileSort(const uint64_t* __restrict__ ids, uint32_t base, uint32_t count,
                                uint64_t* skey, uint32_t* sidx) {
  uint32_t S = 2;
  while (S < count) S <<= 1;
  for (uint32_t i = threadIdx.x; i < S; i += kBlock) {
    skey[i] = i < count ? ids[base + i] : ~0ull;
    sidx[i] = i < count ? base + i : kNone;
  }
  __syncthreads();
  for (uint32_t k = 2; k <= S; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t p = threadIdx.x; p < (S >> 1); p += kBlock) {
        const uint32_t i = 2 * p - (p & (j - 1)), l = i + j;
        const uint64_t ki = skey[i], kl = skey[l];
        const uint32_t ii = sidx[i], il = sidx[l];
        const bool up = (i & k) == 0;
        if (Less(kl, il, ki, ii) == up) {
          skey[i] = kl;
          skey[l] = ki;
          sidx[i] = il;
          sidx[l] = ii;
        }
      }
      __syncthreads();
    }
  }
}

struct EmitOut {
  uint64_t* uniq;
  int64_t* inverse;
  uint32_t* seg;
  int shift;
};

// The tile's `count` sorted elements lie in LDS and start at position base
// of the sorted whole; left is the key at base - 1 (unused at base 0) and
// slot0 the number of heads before the tile. A lane takes kItems
// neighbours. Returns the tile's head count to every lane.
__device__ inline uint32_t EmitTile(const uint64_t* skey, const uint32_t* sidx, uint32_t base,
                                    uint32_t count, uint64_t left, uint32_t slot0, uint32_t* wsum,
                                    EmitOut o) {
  const uint32_t first = threadIdx.x * kItems;
  uint32_t heads = 0;  // bit e: element first + e opens a segment
#pragma unroll
  for (uint32_t e = 0; e < kItems; ++e) {
    const uint32_t i = first + e;
    if (i >= count) break;
    const bool head = i ? skey[i] != skey[i - 1] : (base == 0 || skey[0] != left);
    heads |= static_cast<uint32_t>(head) << e;
  }
  uint32_t total;
  uint32_t slot = slot0 + BlockScan(__popc(heads), wsum, &total);  // heads before this lane's
#pragma unroll
  for (uint32_t e = 0; e < kItems; ++e) {
    const uint32_t i = first + e;
    if (i >= count) break;
    if ((heads >> e) & 1) {
      o.uniq[slot] = skey[i] << o.shift;
      o.seg[slot] = base + i;
      ++slot;
    }
    o.inverse[sidx[i]] = slot - 1;
  }
  return total;
}

// n <= kTile: the whole message in one block
__global__ void __launch_bounds__(kBlock)
    coalesce_small(const uint64_t* __restrict__ ids, uint32_t n, uint32_t* __restrict__ order,
                   uint32_t* __restrict__ m_out, EmitOut o) {
  __shared__ uint64_t skey[kTile];
  __shared__ uint32_t sidx[kTile];
  __shared__ uint32_t wsum[kBlock / 64];
  TileSort(ids, 0, n, skey, sidx);
  for (uint32_t i = threadIdx.x; i < n; i += kBlock) order[i] = sidx[i];
  const uint32_t m = EmitTile(skey, sidx, 0, n, 0, 0, wsum, o);
  if (threadIdx.x == 0) {
    *m_out = m;
    o.seg[m] = n;
  }
}

__global__ void __launch_bounds__(kBlock)
    coalesce_tile_sort(const uint64_t* __restrict__ ids, uint32_t n, uint32_t tiles,
                       uint64_t* __restrict__ keys, uint32_t* __restrict__ order) {
  __shared__ uint64_t skey[kTile];
  __shared__ uint32_t sidx[kTile];
  for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint32_t base = t * kTile;
    const uint32_t count = n - base < kTile ? n - base : kTile;
    TileSort(ids, base, count, skey, sidx);
    for (uint32_t i = threadIdx.x; i < count; i += kBlock) {
      keys[base + i] = skey[i];
      order[base + i] = sidx[i];
    }
    __syncthreads();
  }
}

// Merge path: how many of the first d elements of merge(A, B) come from A.
// A[a] goes before B[b] iff (key, index) of A[a] is the smaller one.
__device__ inline uint32_t MergeCut(const uint64_t* ka, const uint32_t* ia, uint32_t na,
                                    const uint64_t* kb, const uint32_t* ib, uint32_t nb,
                                    uint32_t d) {
  uint32_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1), b = d - 1 - mid;
    if (Less(ka[mid], ia[mid], kb[b], ib[b])) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo;
}

// One pass: sorted runs of `run` elements (a multiple of kTile) are merged
// in pairs; a block makes one tile of output. A last run without a partner
// meets an empty B and is copied by the same code.
__global__ void __launch_bounds__(kBlock)
    coalesce_merge(const uint64_t* __restrict__ keys_in, const uint32_t* __restrict__ order_in,
                   uint64_t* __restrict__ keys_out, uint32_t* __restrict__ order_out, uint32_t n,
                   uint32_t tiles, uint32_t run) {
  __shared__ uint64_t skey[kTile];
  __shared__ uint32_t sidx[kTile];
  __shared__ uint32_t cut[2];
  for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint32_t out0 = t * kTile;
    // run <= 2^30 and out0 < n < 2^31: none of these sums wraps
    const uint32_t a_at = out0 - out0 % (2 * run);  // start of the pair = start of A
    const uint32_t na_all = n - a_at < run ? n - a_at : run;
    const uint32_t b_at = a_at + na_all;
    const uint32_t nb_all = n - b_at < run ? n - b_at : run;
    const uint32_t d0 = out0 - a_at;
    const uint32_t d1 = na_all + nb_all - d0 < kTile ? na_all + nb_all : d0 + kTile;
    // the block's slice of A and of B: two searches in global memory
    if (threadIdx.x == 0 || threadIdx.x == 64) {
      const int which = threadIdx.x >> 6;
      cut[which] = MergeCut(keys_in + a_at, order_in + a_at, na_all, keys_in + b_at,
                            order_in + b_at, nb_all, which ? d1 : d0);
    }
    __syncthreads();
    const uint32_t a0 = cut[0], b0 = d0 - a0;
    const uint32_t na = cut[1] - a0, total = d1 - d0, nb = total - na;
    for (uint32_t i = threadIdx.x; i < total; i += kBlock) {
      const uint32_t src = i < na ? a_at + a0 + i : b_at + b0 + (i - na);
      skey[i] = keys_in[src];
      sidx[i] = order_in[src];
    }
    __syncthreads();
    // a lane's kItems outputs: its own cut in LDS, then a serial merge
    const uint32_t d = threadIdx.x * kItems < total ? threadIdx.x * kItems : total;
    uint32_t a = MergeCut(skey, sidx, na, skey + na, sidx + na, nb, d);
    uint32_t b = na + d - a;  // B's elements follow A's in LDS
    uint64_t ok[kItems];
    uint32_t oi[kItems];
    uint64_t ka = a < na ? skey[a] : 0, kb = b < total ? skey[b] : 0;
    uint32_t ia = a < na ? sidx[a] : 0, ib = b < total ? sidx[b] : 0;
#pragma unroll
    for (uint32_t e = 0; e < kItems; ++e) {
      if (d + e >= total) break;
      const bool take_a = b >= total || (a < na && Less(ka, ia, kb, ib));
      ok[e] = take_a ? ka : kb;
      oi[e] = take_a ? ia : ib;
      if (take_a) {
        ++a;
        if (a < na) {
          ka = skey[a];
          ia = sidx[a];
        }
      } else {
        ++b;
        if (b < total) {
          kb = skey[b];
          ib = sidx[b];
        }
      }
    }
    __syncthreads();
    // through LDS once more so that the stores to global memory are dense
#pragma unroll
    for (uint32_t e = 0; e < kItems; ++e) {
      if (d + e >= total) break;
      skey[d + e] = ok[e];
      sidx[d + e] = oi[e];
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < total; i += kBlock) {
      keys_out[out0 + i] = skey[i];
      order_out[out0 + i] = sidx[i];
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kBlock)
    coalesce_count_heads(const uint64_t* __restrict__ keys, uint32_t n, uint32_t tiles,
                         uint32_t* __restrict__ tile_heads) {
  __shared__ uint32_t wsum[kBlock / 64];
  for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint32_t base = t * kTile;
    const uint32_t count = n - base < kTile ? n - base : kTile;
    uint32_t heads = 0;
    for (uint32_t i = threadIdx.x; i < count; i += kBlock) {
      const uint32_t at = base + i;
      heads += at == 0 || keys[at] != keys[at - 1];
    }
    uint32_t total;
    BlockScan(heads, wsum, &total);
    if (threadIdx.x == 0) tile_heads[t] = total;
  }
}

// one block: tile_heads becomes its own exclusive scan, *m_out the sum
__global__ void __launch_bounds__(kBlock)
    coalesce_scan_tiles(uint32_t* __restrict__ tile_heads, uint32_t tiles, uint32_t n,
                        uint32_t* __restrict__ m_out, uint32_t* __restrict__ seg) {
  __shared__ uint32_t wsum[kBlock / 64];
  uint32_t carry = 0;
  for (uint32_t c = 0; c < tiles; c += kBlock) {
    const uint32_t t = c + threadIdx.x;
    const uint32_t v = t < tiles ? tile_heads[t] : 0;
    uint32_t total;
    const uint32_t before = BlockScan(v, wsum, &total);
    if (t < tiles) tile_heads[t] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) {
    *m_out = carry;
    seg[carry] = n;
  }
}

__global__ void __launch_bounds__(kBlock)
    coalesce_emit(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ order, uint32_t n,
                  uint32_t tiles, const uint32_t* __restrict__ tile_slot0, EmitOut o) {
  __shared__ uint64_t skey[kTile];
  __shared__ uint32_t sidx[kTile];
  __shared__ uint32_t wsum[kBlock / 64];
  for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint32_t base = t * kTile;
    const uint32_t count = n - base < kTile ? n - base : kTile;
    for (uint32_t i = threadIdx.x; i < count; i += kBlock) {
      skey[i] = keys[base + i];
      sidx[i] = order[base + i];
    }
    __syncthreads();
    EmitTile(skey, sidx, base, count, base ? keys[base - 1] : 0, tile_slot0[t], wsum, o);
    __syncthreads();
  }
}

struct Float8 {
  float4 lo, hi;
};
__device__ inline float Add(float a, float b) { return a + b; }
__device__ inline float4 Add(float4 a, float4 b) {
  return float4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
}
__device__ inline Float8 Add(Float8 a, Float8 b) {
  return Float8{Add(a.lo, b.lo), Add(a.hi, b.hi)};
}

// round-to-nearest-even to bf16 bits, sparse_bf16.hip's nearest rule: Inf as
// it is, a NaN keeps a mantissa bit
__device__ inline uint32_t Bf16(float x) {
  const uint32_t u = __float_as_uint(x);
  uint32_t h = u >> 16;
  if ((u & 0x7f800000u) == 0x7f800000u) {
    if ((h & 0x7fu) == 0 && (u & 0xffffu)) h |= 0x40u;
    return h;
  }
  return (u + 0x7fffu + (h & 1u)) >> 16;
}
__device__ inline uint32_t Bf16x2(float a, float b) { return Bf16(a) | (Bf16(b) << 16); }

// a row sum on its way out: as it is, or as bf16 bits (8 of them: one 16 B store)
__device__ inline void Put(float* p, float v) { *p = v; }
__device__ inline void Put(float4* p, float4 v) { *p = v; }
__device__ inline void Put(uint16_t* p, float v) { *p = static_cast<uint16_t>(Bf16(v)); }
__device__ inline void Put(uint4* p, Float8 v) {
  *p = uint4{Bf16x2(v.lo.x, v.lo.y), Bf16x2(v.lo.z, v.lo.w), Bf16x2(v.hi.x, v.hi.y),
             Bf16x2(v.hi.z, v.hi.w)};
}

// sums[slot] = +0.0 + grad[i] over the slot's occurrences i < grad_rows in
// ascending i. A group of G = 1 << log2g lanes owns a slot and walks its
// segment of the sorted index array once per G vectors of the row; the
// rows of kAhead occurrences are in flight before the first of their adds.
// V is a lane's vector of the gradient, S what it stores of the sums.
template <class V, class S>
__global__ void __launch_bounds__(kBlock)
    coalesce_row_sums(const V* __restrict__ grad, S* __restrict__ sums,
                      const uint32_t* __restrict__ seg, const uint32_t* __restrict__ order,
                      const uint32_t* __restrict__ m_dev, uint32_t grad_rows, size_t nv,
                      int log2g) {
  const uint32_t G = 1u << log2g;
  const uint32_t lane = threadIdx.x & 63, gl = lane & (G - 1);
  const size_t per_wave = 64 >> log2g;
  const size_t wave = (blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x) >> 6;
  const size_t nwaves = (static_cast<size_t>(gridDim.x) * blockDim.x) >> 6;
  const uint32_t m = *m_dev;
  for (size_t first = wave * per_wave; first < m; first += nwaves * per_wave) {
    const size_t slot = first + (lane >> log2g);
    if (slot >= m) return;  // nothing below crosses lanes
    const uint32_t lo = seg[slot], hi = seg[slot + 1];
    for (size_t c = gl; c < nv; c += G) {
      V acc{};
      uint32_t i[kAhead], next[kAhead];
#pragma unroll
      for (int k = 0; k < kAhead; ++k) i[k] = lo + k < hi ? order[lo + k] : kNone;
      for (uint32_t j = lo; j < hi; j += kAhead) {
        V v[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
          if (i[k] < grad_rows) v[k] = grad[i[k] * nv + c];
        }
        // indices ascend: a last one without a gradient ends the walk
        const bool more = i[kAhead - 1] < grad_rows;
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {  // the next indices travel with these rows
          next[k] = more && j + kAhead + k < hi ? order[j + kAhead + k] : kNone;
        }
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
          if (i[k] < grad_rows) acc = Add(acc, v[k]);
        }
        if (!more) break;
#pragma unroll
        for (int k = 0; k < kAhead; ++k) i[k] = next[k];
      }
      Put(sums + slot * nv + c, acc);
    }
  }
}

template <class V, class S, class T>
void LaunchRowSums(const float* grad, T* sums, const uint32_t* seg, const uint32_t* order,
                   const uint32_t* m_dev, size_t n, size_t grad_rows, size_t nv, int grid_cap,
                   hipStream_t s) {
  int log2g = 0;
  while ((size_t{1} << log2g) < nv && log2g < 6) ++log2g;
  // m is still on the device: the grid is sized for n slots and waves past m leave
  size_t per_wave = 64 >> log2g;
  size_t waves = (n + per_wave - 1) / per_wave;
  int grid = GridFor(waves * 64, 16384, grid_cap);
  hipLaunchKernelGGL((coalesce_row_sums<V, S>), dim3(grid), dim3(kBlock), 0, s,
                     reinterpret_cast<const V*>(grad), reinterpret_cast<S*>(sums), seg, order,
                     m_dev, static_cast<uint32_t>(grad_rows), nv, log2g);
}

inline size_t Round16(size_t b) { return (b + 15) & ~size_t{15}; }

// the workspace, cut at 16 B boundaries
struct Workspace {
  uint64_t* keys[2];
  uint32_t* order[2];
  uint32_t* seg;         // n + 1
  uint32_t* tile_heads;  // tiles
  uint32_t* m;
  size_t bytes;  // from the aligned base
  Workspace(uintptr_t base, size_t n) {
    size_t tiles = (n + kTile - 1) / kTile;
    uintptr_t p = base;
    auto take = [&p](size_t b) {
      uintptr_t at = p;
      p += Round16(b);
      return at;
    };
    for (auto& k : keys) k = reinterpret_cast<uint64_t*>(take(n * 8));
    for (auto& o : order) o = reinterpret_cast<uint32_t*>(take(n * 4));
    seg = reinterpret_cast<uint32_t*>(take((n + 1) * 4));
    tile_heads = reinterpret_cast<uint32_t*>(take(tiles * 4));
    m = reinterpret_cast<uint32_t*>(take(4));
    bytes = p - base;
  }
};

template <class... Ptrs>
inline bool Aligned8(const Ptrs*... p) {
  return ((reinterpret_cast<uintptr_t>(p) | ...) & 7u) == 0;
}

// the row sums of a coalesced message, in the widest vectors the call admits
void RowSums(const float* grad, float* sums, const Workspace& w, const uint32_t* order, size_t n,
             size_t with_grad, size_t row_len, int grid_cap, hipStream_t s) {
  // float4 needs whole vectors and both arrays on a 16 B boundary
  if (row_len % 4 == 0 && Aligned16(grad, sums)) {
    LaunchRowSums<float4, float4>(grad, sums, w.seg, order, w.m, n, with_grad, row_len / 4,
                                  grid_cap, s);
  } else {
    LaunchRowSums<float, float>(grad, sums, w.seg, order, w.m, n, with_grad, row_len, grid_cap, s);
  }
}
void RowSums(const float* grad, uint16_t* sums, const Workspace& w, const uint32_t* order, size_t n,
             size_t with_grad, size_t row_len, int grid_cap, hipStream_t s) {
  // 8 sums are one 16 B store: whole units and both arrays on a 16 B boundary
  if (row_len % 8 == 0 && Aligned16(grad) && Aligned16(sums)) {
    LaunchRowSums<Float8, uint4>(grad, sums, w.seg, order, w.m, n, with_grad, row_len / 8,
                                 grid_cap, s);
  } else {
    LaunchRowSums<float, uint16_t>(grad, sums, w.seg, order, w.m, n, with_grad, row_len, grid_cap,
                                   s);
  }
}

}  // namespace

int SparseCoalesceTile() { return kTile; }

size_t SparseCoalesceWorkspaceBytes(size_t n) {
  return Workspace(0, n).bytes + 16;  // the caller's pointer may sit anywhere in 16 B
}

namespace {

template <class T>
size_t Coalesce(const uint64_t* ids_dev, size_t n, int key_shift, const float* grad_or_null,
                size_t grad_rows, size_t row_len, uint64_t* uniq_keys, T* sums_or_null,
                int64_t* inverse, void* workspace, size_t workspace_bytes, hipStream_t s,
                int grid_cap) {
  if (n >= (size_t{1} << 31)) throw std::invalid_argument("SparseCoalesce: n must be below 2^31");
  if (grad_rows > n) throw std::invalid_argument("SparseCoalesce: grad_rows exceeds n");
  if (grad_or_null && row_len == 0) {
    throw std::invalid_argument("SparseCoalesce: a gradient needs row_len > 0");
  }
  if (key_shift < 0 || key_shift > 63) {
    throw std::invalid_argument("SparseCoalesce: key_shift must lie in [0, 63]");
  }
  if (!Aligned8(ids_dev, uniq_keys, inverse)) {
    throw std::invalid_argument("SparseCoalesce: ids, uniq_keys and inverse need 8 B alignment");
  }
  if (workspace_bytes < SparseCoalesceWorkspaceBytes(n)) {
    throw std::invalid_argument("SparseCoalesce: workspace below SparseCoalesceWorkspaceBytes(n)");
  }
  if (n == 0) return 0;

  const Workspace w((reinterpret_cast<uintptr_t>(workspace) + 15) & ~uintptr_t{15}, n);
  const uint32_t n32 = static_cast<uint32_t>(n);
  const uint32_t tiles = (n32 + kTile - 1) / kTile;
  const EmitOut emit{uniq_keys, inverse, w.seg, key_shift};
  const uint32_t* order = w.order[0];
  if (tiles == 1) {
    hipLaunchKernelGGL(coalesce_small, dim3(1), dim3(kBlock), 0, s, ids_dev, n32, w.order[0], w.m,
                       emit);
  } else {
    // one block per tile: a tile is a block's worth of LDS whatever the grid
    const dim3 grid(GridFor(size_t{tiles} * kBlock, 1 << 22, grid_cap)), block(kBlock);
    hipLaunchKernelGGL(coalesce_tile_sort, grid, block, 0, s, ids_dev, n32, tiles, w.keys[0],
                       w.order[0]);
    int from = 0;
    for (uint64_t run = kTile; run < n; run <<= 1, from ^= 1) {
      hipLaunchKernelGGL(coalesce_merge, grid, block, 0, s, w.keys[from], w.order[from],
                         w.keys[from ^ 1], w.order[from ^ 1], n32, tiles,
                         static_cast<uint32_t>(run));
    }
    order = w.order[from];
    hipLaunchKernelGGL(coalesce_count_heads, grid, block, 0, s, w.keys[from], n32, tiles,
                       w.tile_heads);
    hipLaunchKernelGGL(coalesce_scan_tiles, dim3(1), block, 0, s, w.tile_heads, tiles, n32, w.m,
                       w.seg);
    hipLaunchKernelGGL(coalesce_emit, grid, block, 0, s, w.keys[from], order, n32, tiles,
                       w.tile_heads, emit);
  }
  if (sums_or_null && row_len) {
    RowSums(grad_or_null, sums_or_null, w, order, n, grad_or_null ? grad_rows : 0, row_len,
            grid_cap, s);
  }
  uint32_t m = 0;
  hipError_t e = hipMemcpyAsync(&m, w.m, sizeof(m), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    throw std::runtime_error(std::string("SparseCoalesce: ") + hipGetErrorString(e));
  }
  return m;
}

}  // namespace

size_t SparseCoalesce(const uint64_t* ids_dev, size_t n, int key_shift, const float* grad_or_null,
                      size_t grad_rows, size_t row_len, uint64_t* uniq_keys, float* sums_or_null,
                      int64_t* inverse, void* workspace, size_t workspace_bytes, hipStream_t s,
                      int grid_cap) {
  return Coalesce(ids_dev, n, key_shift, grad_or_null, grad_rows, row_len, uniq_keys, sums_or_null,
                  inverse, workspace, workspace_bytes, s, grid_cap);
}
size_t SparseCoalesceBf16(const uint64_t* ids_dev, size_t n, int key_shift,
                          const float* grad_or_null, size_t grad_rows, size_t row_len,
                          uint64_t* uniq_keys, uint16_t* sums_or_null, int64_t* inverse,
                          void* workspace, size_t workspace_bytes, hipStream_t s, int grid_cap) {
  return Coalesce(ids_dev, n, key_shift, grad_or_null, grad_rows, row_len, uniq_keys, sums_or_null,
                  inverse, workspace, workspace_bytes, s, grid_cap);
}

}  // namespace kern
}  // namespace xps
