// CDNA4 (gfx950) kernels for the KVServer request handlers.
//
// All kernels are HBM-bandwidth-bound streaming ops, so the design rules
// are (cdna_hip_programming.md §2): 16 B per lane per instruction
// (uint4/float4), 64-wide wavefronts, grid-stride loops sized >> 256
// workgroups to fill 8 XCDs, and a single pass over dst for the
// multi-source reduction. Inputs may be hipIpc-mapped peer-GPU memory —
// the loads then ride xGMI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "kernels.h"
#include "tile_runs.h"

namespace xps {
namespace kern {

namespace {

constexpr int kBlock = 256;

inline int GridFor(size_t work_items, int cap = 8192) {
  size_t g = (work_items + kBlock - 1) / kBlock;
  if (g > static_cast<size_t>(cap)) g = cap;
  if (g == 0) g = 1;
  return static_cast<int>(g);
}

// test-only grid caps (grid_cap / tile_cap arguments): 0 leaves the grid as is
inline int CapGrid(int grid, int cap) { return cap > 0 && grid > cap ? cap : grid; }

// NOTE: nontemporal loads/stores were measured 3 % SLOWER end-to-end
// here, with the push and the pull as two kernels (the pull re-read the
// just-written store). Keep plain float4. For the dual-write kernels
// below, which have no such re-read, the hints were measured again and
// lost again (see batched_assign2_kernel).
__global__ void assign_kernel(uint4* __restrict__ dst, const uint4* __restrict__ src, size_t n4) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < n4; i += stride) dst[i] = src[i];
}

// The element kernels (bytes here, floats and bf16 below) serve two
// launches: one block for the sub-16 B tail [n4 * 16, nbytes) of an
// aligned range, and a grid-stride sweep of a whole range [0, n) whose
// pointers are not 16 B-aligned.
__global__ void assign_tail_kernel(char* __restrict__ dst, const char* __restrict__ src,
                                   size_t begin, size_t end) {
  size_t i = begin + blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < end; i += stride) dst[i] = src[i];
}

// Fused push+pull of one key: one 16 B load per lane per iteration, two
// 16 B stores (store entry + the requester's pull destination). Moves
// 3 bytes of traffic per payload byte where the assign_kernel pair moved
// 4, in one launch. The three ranges must be pairwise disjoint. The
// sub-16 B tail [tail_begin, nbytes) rides the same launch as a byte
// grid-stride loop; launched with n4 == 0 and tail_begin == 0 that loop
// copies a whole (misaligned) range.
// Plain stores, no unrolling — same-session A/B on the 128 x 64 MiB
// headline, 3 alternating runs each (profiles/dense64_fused_rocprof.md):
// this kernel 3283-3428 GB/s; nontemporal store to the store entry (no
// longer re-read by this round's pull) 3327-3397, inside that spread, so
// not adopted; 2 loads in flight per lane 3026-3069 and 2 loads + nt
// 3226-3244, both slower; 4 loads in flight 3294-3401, no gain.
// The sweep behind the batched kernel's 8 KiB tiles
// (profiles/dense64_dualwrite_rocprof.md) left this kernel as it is: its
// loop already has uniform pointers and issues the next load ahead of the
// wait on the stores, and one 64 MiB key is 8192 blocks of two strides
// each, the geometry the sweep chose, swept as a grid stride where the
// batched kernel sweeps a tile. It runs from two processes at once in the
// shared-GPU config, which was not to be disturbed.
__global__ void assign2_kernel(uint4* __restrict__ dst0, uint4* __restrict__ dst1,
                               const uint4* __restrict__ src, size_t n4, size_t tail_begin,
                               size_t nbytes) {
  size_t tid = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = tid; i < n4; i += stride) {
    uint4 v = src[i];
    dst0[i] = v;
    dst1[i] = v;
  }
  char* b0 = reinterpret_cast<char*>(dst0);
  char* b1 = reinterpret_cast<char*>(dst1);
  const char* bs = reinterpret_cast<const char*>(src);
  for (size_t i = tail_begin + tid; i < nbytes; i += stride) {
    char c = bs[i];
    b0[i] = c;
    b1[i] = c;
  }
}

__global__ void sum_kernel_f32(float4* __restrict__ dst, const float4* __restrict__ src,
                               size_t n4) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < n4; i += stride) {
    float4 d = dst[i];
    float4 s = src[i];
    d.x += s.x;
    d.y += s.y;
    d.z += s.z;
    d.w += s.w;
    dst[i] = d;
  }
}

__global__ void sum_tail_f32(float* __restrict__ dst, const float* __restrict__ src, size_t begin,
                             size_t end) {
  size_t i = begin + blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < end; i += stride) dst[i] += src[i];
}

// bf16 += bf16 with fp32 accumulate in-register, 16 B per lane (8 bf16
// elements via uint4). bf16 -> fp32 is a 16-bit shift; fp32 -> bf16
// rounds to nearest-even (matches torch's bf16 semantics).
__device__ inline float bf16_to_f32(uint16_t h) {
  union {
    uint32_t u;
    float f;
  } c;
  c.u = static_cast<uint32_t>(h) << 16;
  return c.f;
}

__device__ inline uint16_t f32_to_bf16(float f) {
  union {
    uint32_t u;
    float f;
  } c;
  c.f = f;
  uint32_t lsb = (c.u >> 16) & 1u;
  return static_cast<uint16_t>((c.u + 0x7FFFu + lsb) >> 16);
}

__device__ inline uint32_t bf16x2_sum(uint32_t d, uint32_t s) {
  float lo = bf16_to_f32(static_cast<uint16_t>(d)) + bf16_to_f32(static_cast<uint16_t>(s));
  float hi = bf16_to_f32(static_cast<uint16_t>(d >> 16)) +
             bf16_to_f32(static_cast<uint16_t>(s >> 16));
  return static_cast<uint32_t>(f32_to_bf16(lo)) |
         (static_cast<uint32_t>(f32_to_bf16(hi)) << 16);
}

__global__ void sum_kernel_bf16(uint4* __restrict__ dst, const uint4* __restrict__ src,
                                size_t n8) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < n8; i += stride) {
    uint4 d = dst[i];
    uint4 s = src[i];
    d.x = bf16x2_sum(d.x, s.x);
    d.y = bf16x2_sum(d.y, s.y);
    d.z = bf16x2_sum(d.z, s.z);
    d.w = bf16x2_sum(d.w, s.w);
    dst[i] = d;
  }
}

__global__ void sum_tail_bf16(uint16_t* __restrict__ dst, const uint16_t* __restrict__ src,
                              size_t begin, size_t end) {
  size_t i = begin + blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < end; i += stride) {
    dst[i] = f32_to_bf16(bf16_to_f32(dst[i]) + bf16_to_f32(src[i]));
  }
}

// flat indexing: thread i handles element i of the CONCATENATED rows
// (row = i / row_len4), so narrow rows (e.g. 64 floats = 16 float4)
// still use every lane — a row-per-block mapping left 94 % of the block
// idle at width 64.
// Every kernel bounds-checks the decoded local row against tab_rows: a
// misrouted or corrupt key must not scribble over the shared pool (or a
// hipIpc-mapped peer). The unsigned compare also catches keys below
// row_base (the subtraction wraps to a huge value). Gather returns
// zeros for such rows (defined output); scatters skip them.
__global__ void gather_rows_f32(const float4* __restrict__ table, const uint64_t* __restrict__ rows,
                                size_t nrows, size_t row_len4, float4* __restrict__ out,
                                int shift, uint64_t base, uint64_t tab_rows) {
  size_t total = nrows * row_len4;
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < total; i += stride) {
    size_t r = i / row_len4;
    size_t c = i - r * row_len4;
    uint64_t row = (rows[r] >> shift) - base;
    out[i] = row < tab_rows ? table[row * row_len4 + c] : float4{0.f, 0.f, 0.f, 0.f};
  }
}

__global__ void scatter_add_rows_f32(float4* __restrict__ table, const uint64_t* __restrict__ rows,
                                     size_t nrows, size_t row_len4,
                                     const float4* __restrict__ src, int shift, uint64_t base,
                                     uint64_t tab_rows) {
  size_t total = nrows * row_len4;
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < total; i += stride) {
    size_t r = i / row_len4;
    size_t c = i - r * row_len4;
    uint64_t row = (rows[r] >> shift) - base;
    if (row >= tab_rows) continue;
    float4* dst = table + row * row_len4 + c;
    float4 d = *dst;
    float4 v = src[i];
    d.x += v.x;
    d.y += v.y;
    d.z += v.z;
    d.w += v.w;
    *dst = d;
  }
}

__global__ void gather_rows_scalar_f32(const float* __restrict__ table,
                                       const uint64_t* __restrict__ rows, size_t nrows,
                                       size_t row_len, float* __restrict__ out, int shift,
                                       uint64_t base, uint64_t tab_rows) {
  for (size_t r = blockIdx.x; r < nrows; r += gridDim.x) {
    uint64_t row = (rows[r] >> shift) - base;
    const float* src = table + row * row_len;
    float* dst = out + r * row_len;
    for (size_t c = threadIdx.x; c < row_len; c += blockDim.x) {
      dst[c] = row < tab_rows ? src[c] : 0.f;
    }
  }
}

__global__ void scatter_assign_rows_f32(float4* __restrict__ table,
                                        const uint64_t* __restrict__ rows, size_t nrows,
                                        size_t row_len4, const float4* __restrict__ src,
                                        int shift, uint64_t base, uint64_t tab_rows) {
  size_t total = nrows * row_len4;
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < total; i += stride) {
    size_t r = i / row_len4;
    size_t c = i - r * row_len4;
    uint64_t row = (rows[r] >> shift) - base;
    if (row < tab_rows) table[row * row_len4 + c] = src[i];
  }
}

__global__ void scatter_assign_rows_scalar_f32(float* __restrict__ table,
                                               const uint64_t* __restrict__ rows, size_t nrows,
                                               size_t row_len, const float* __restrict__ src,
                                               int shift, uint64_t base, uint64_t tab_rows) {
  for (size_t r = blockIdx.x; r < nrows; r += gridDim.x) {
    uint64_t row = (rows[r] >> shift) - base;
    if (row >= tab_rows) continue;
    float* dst = table + row * row_len;
    const float* s = src + r * row_len;
    for (size_t c = threadIdx.x; c < row_len; c += blockDim.x) dst[c] = s[c];
  }
}

__global__ void scatter_add_rows_atomic_f32(float* __restrict__ table,
                                            const uint64_t* __restrict__ rows, size_t nrows,
                                            size_t row_len, const float* __restrict__ src,
                                            int shift, uint64_t base, uint64_t tab_rows) {
  for (size_t r = blockIdx.x; r < nrows; r += gridDim.x) {
    uint64_t row = (rows[r] >> shift) - base;
    if (row >= tab_rows) continue;
    float* dst = table + row * row_len;
    const float* s = src + r * row_len;
    for (size_t c = threadIdx.x; c < row_len; c += blockDim.x) {
      atomicAdd(&dst[c], s[c]);
    }
  }
}

struct DescArray {
  CopyDesc d[kMaxBatch];
  int n;
};

// balanced variant: segments are concatenated into one virtual chunk
// space (prefix = exclusive 16-B-chunk offsets); each BLOCK owns
// contiguous tiles of that space, so work splits evenly across mixed
// segment sizes (the per-segment grid-stride left small buckets on a
// handful of blocks while every block swept all 64 segment headers).
// Within a tile lanes stay consecutive (coalesced); the tile's segment
// is found once and walked forward.
struct BalancedDescArray {
  CopyDesc d[kMaxBatch];
  unsigned long long prefix[kMaxBatch + 1];  // chunk offsets, prefix[n] = total
  int n;
};

// kOp: 0 = byte assign, 1 = fp32 sum, 2 = bf16 sum (fp32 accumulate)
template <int kOp>
__global__ void batched_balanced_kernel(BalancedDescArray da, size_t chunks_per_block) {
  size_t total = da.prefix[da.n];
  size_t tile_begin = blockIdx.x * chunks_per_block;
  size_t tile_end = tile_begin + chunks_per_block;
  if (tile_end > total) tile_end = total;
  if (tile_begin >= total) return;
  // locate the first segment of this tile (binary search once)
  int seg = 0;
  {
    int lo = 0, hi = da.n - 1;
    while (lo < hi) {
      int mid = (lo + hi + 1) >> 1;
      if (da.prefix[mid] <= tile_begin) {
        lo = mid;
      } else {
        hi = mid - 1;
      }
    }
    seg = lo;
  }
  for (size_t g = tile_begin + threadIdx.x; g < tile_end; g += blockDim.x) {
    while (g >= da.prefix[seg + 1]) ++seg;  // walk forward (tiles are contiguous)
    size_t local = g - da.prefix[seg];
    if (kOp == 1) {
      float4* dst = reinterpret_cast<float4*>(da.d[seg].dst) + local;
      const float4* src = reinterpret_cast<const float4*>(da.d[seg].src) + local;
      float4 a = *dst;
      float4 b = *src;
      a.x += b.x;
      a.y += b.y;
      a.z += b.z;
      a.w += b.w;
      *dst = a;
    } else if (kOp == 2) {
      uint4* dst = reinterpret_cast<uint4*>(da.d[seg].dst) + local;
      const uint4* src = reinterpret_cast<const uint4*>(da.d[seg].src) + local;
      uint4 a = *dst;
      uint4 b = *src;
      a.x = bf16x2_sum(a.x, b.x);
      a.y = bf16x2_sum(a.y, b.y);
      a.z = bf16x2_sum(a.z, b.z);
      a.w = bf16x2_sum(a.w, b.w);
      *dst = a;
    } else {
      reinterpret_cast<uint4*>(da.d[seg].dst)[local] =
          reinterpret_cast<const uint4*>(da.d[seg].src)[local];
    }
  }
}

struct Seg2Array {
  Seg2 d[kMaxBatch];
  unsigned long long prefix[kMaxBatch + 1];  // chunk offsets, prefix[n] = total
  int n;
};

// Dual-write counterpart of the balanced kernel: up to kMaxBatch fused
// push+pull segments concatenated in the 16 B-chunk prefix space, one
// 16 B load and two 16 B stores per lane per iteration. No segment is
// empty, so prefix is strictly increasing.
// Each block owns one contiguous tile of chunks_per_block chunks and
// takes it apart into runs, one per segment the tile touches
// (tile_runs.h). The run list comes from block-uniform values only, so
// the segment table is read with scalar loads and the inner loop has
// uniform base pointers: the next load is issued while the previous
// iteration's stores are still in flight. (The earlier form let every
// lane walk the segment list; its loop waited for the stores to drain
// ahead of each load.)
// What was measured (profiles/dense64_dualwrite_rocprof.md; one process,
// 16 x 64 MiB per launch, variants interleaved, µs per 64 MiB key on the
// slower / faster of two buffer sets):
//   per-lane walk, 128 KiB tiles (the shape before)   39.9 / 34.5
//   runs, 128 KiB tiles                               37.8 / 34.1
//   runs, 8 KiB tiles (shipped)                       32.9 / 31.6
// Tile size is the axis that pays: 4-16 KiB are level, 32 KiB is 1 µs
// behind, 64 KiB and up fall back to the old figure. 2, 4 or 8 loads in
// flight per lane, blocks of 512 or 1024, a fixed grid of 256*k blocks
// looping over tiles, a non-power-of-two tile, a rotated start inside
// the tile and nontemporal hints on any of the three streams were each
// inside the noise or slower, so none of them is here.
constexpr size_t kTileChunks2 = 512;  // 8 KiB per block, two strides of the block

__global__ void __launch_bounds__(kBlock)
    batched_assign2_kernel(Seg2Array da, size_t chunks_per_block) {
  TileRunIter it = TileRunsBegin(da.prefix, da.n, chunks_per_block, blockIdx.x);
  TileRun run;
  while (TileRunsNext(da.prefix, &it, &run)) {
    uint4* __restrict__ d0 = static_cast<uint4*>(da.d[run.seg].dst0);
    uint4* __restrict__ d1 = static_cast<uint4*>(da.d[run.seg].dst1);
    const uint4* __restrict__ sp = static_cast<const uint4*>(da.d[run.seg].src);
    for (size_t i = run.lo + threadIdx.x; i < run.hi; i += kBlock) {
      uint4 v = sp[i];
      d0[i] = v;
      d1[i] = v;
    }
  }
}

// every block strides over every segment's 16B chunks (grid sized for
// the concatenated total, so all segments together fill the 8 XCDs)
// (segment loop per block; fine for <= kMaxBatch segments)
__global__ void batched_assign_kernel(DescArray da) {
  for (int seg = 0; seg < da.n; ++seg) {
    uint4* dst = reinterpret_cast<uint4*>(da.d[seg].dst);
    const uint4* src = reinterpret_cast<const uint4*>(da.d[seg].src);
    size_t n4 = da.d[seg].nbytes / 16;
    size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
    size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (; i < n4; i += stride) dst[i] = src[i];
  }
}

__global__ void batched_sum_kernel_bf16(DescArray da) {
  for (int seg = 0; seg < da.n; ++seg) {
    uint4* dst = reinterpret_cast<uint4*>(da.d[seg].dst);
    const uint4* src = reinterpret_cast<const uint4*>(da.d[seg].src);
    size_t n8 = da.d[seg].nbytes / 16;
    size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
    size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (; i < n8; i += stride) {
      uint4 d = dst[i];
      uint4 s = src[i];
      d.x = bf16x2_sum(d.x, s.x);
      d.y = bf16x2_sum(d.y, s.y);
      d.z = bf16x2_sum(d.z, s.z);
      d.w = bf16x2_sum(d.w, s.w);
      dst[i] = d;
    }
  }
}

__global__ void batched_sum_kernel_f32(DescArray da) {
  for (int seg = 0; seg < da.n; ++seg) {
    float4* dst = reinterpret_cast<float4*>(da.d[seg].dst);
    const float4* src = reinterpret_cast<const float4*>(da.d[seg].src);
    size_t n4 = da.d[seg].nbytes / 16;
    size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
    size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (; i < n4; i += stride) {
      float4 d = dst[i];
      float4 v = src[i];
      d.x += v.x;
      d.y += v.y;
      d.z += v.z;
      d.w += v.w;
      dst[i] = d;
    }
  }
}

}  // namespace

namespace {

bool BalancedBatchEnabled() {
  static const bool on = [] {
    const char* v = getenv("XPS_BALANCED_BATCH");
    return !v || atoi(v) != 0;  // default on
  }();
  return on;
}

template <int kOp>
void LaunchBalanced(const CopyDesc* descs_host, int n, hipStream_t s, int tile_cap) {
  size_t max_blocks = tile_cap > 0 ? std::min(tile_cap, 8192) : 8192;
  for (int off = 0; off < n; off += kMaxBatch) {
    BalancedDescArray da{};
    da.n = std::min(n - off, kMaxBatch);
    unsigned long long acc = 0;
    for (int i = 0; i < da.n; ++i) {
      da.d[i] = descs_host[off + i];
      da.prefix[i] = acc;
      acc += da.d[i].nbytes / 16;
    }
    da.prefix[da.n] = acc;
    if (acc == 0) continue;
    // tile size: fill ~8192 blocks (8 XCDs want >> 256 workgroups),
    // whole multiples of the block so lanes sweep full strides (under a
    // tile_cap the tile grows and a block sweeps several strides of it)
    size_t cpb = (acc + max_blocks - 1) / max_blocks;
    cpb = ((cpb + kBlock - 1) / kBlock) * kBlock;
    int grid = static_cast<int>((acc + cpb - 1) / cpb);
    hipLaunchKernelGGL((batched_balanced_kernel<kOp>), dim3(grid), dim3(kBlock), 0, s, da,
                       cpb);
  }
}

// XPS_BALANCED_BATCH=0: every block strides over every segment, the grid
// sized for the concatenated total
template <typename Kernel>
void LaunchLegacy(Kernel kernel, const CopyDesc* descs_host, int n, hipStream_t s,
                  int tile_cap) {
  size_t total = 0;
  for (int i = 0; i < n; ++i) total += descs_host[i].nbytes;
  if (total < 16) return;  // nothing but empty segments
  int grid = CapGrid(GridFor(total / 16), tile_cap);
  DescArray da{};
  for (int off = 0; off < n; off += kMaxBatch) {
    da.n = std::min(n - off, kMaxBatch);
    for (int i = 0; i < da.n; ++i) da.d[i] = descs_host[off + i];
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, s, da);
  }
}

// the 16 B kernels need both pointers 16 B-aligned (pool buffers are);
// anything else takes the element kernel for the whole range
inline bool Aligned16(const void* a, const void* b) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0;
}

}  // namespace

void BatchedAssign(const CopyDesc* descs_host, int n, hipStream_t s, int tile_cap) {
  if (BalancedBatchEnabled()) {
    LaunchBalanced<0>(descs_host, n, s, tile_cap);
    return;
  }
  LaunchLegacy(batched_assign_kernel, descs_host, n, s, tile_cap);
}

void BatchedAssign2(const Seg2* segs_host, int n, hipStream_t s, int tile_cap) {
  int max_blocks = tile_cap > 0 ? std::min(tile_cap, 8192) : 8192;
  int off = 0;
  while (off < n) {
    Seg2Array da{};
    unsigned long long acc = 0;
    while (off < n && da.n < kMaxBatch) {
      const Seg2& sg = segs_host[off++];
      if (sg.nbytes < 16) continue;  // keeps prefix strictly increasing
      da.d[da.n] = sg;
      da.prefix[da.n] = acc;
      acc += sg.nbytes / 16;
      ++da.n;
    }
    da.prefix[da.n] = acc;
    if (acc == 0) continue;
    // tile size: whole multiples of the block so lanes sweep full
    // strides, enough for ~8192 blocks on a small launch, and no more
    // than kTileChunks2 however large the launch (past 64 MiB the grid
    // grows instead of the tile). A tile_cap is obeyed as given.
    size_t cpb = (acc + max_blocks - 1) / max_blocks;
    cpb = ((cpb + kBlock - 1) / kBlock) * kBlock;
    if (tile_cap <= 0 && cpb > kTileChunks2) cpb = kTileChunks2;
    int grid = static_cast<int>((acc + cpb - 1) / cpb);
    hipLaunchKernelGGL(batched_assign2_kernel, dim3(grid), dim3(kBlock), 0, s, da, cpb);
  }
}

void BatchedSumF32(const CopyDesc* descs_host, int n, hipStream_t s, int tile_cap) {
  if (BalancedBatchEnabled()) {
    LaunchBalanced<1>(descs_host, n, s, tile_cap);
    return;
  }
  LaunchLegacy(batched_sum_kernel_f32, descs_host, n, s, tile_cap);
}

void DenseAssign(void* dst, const void* src, size_t nbytes, hipStream_t s, int grid_cap) {
  if (!Aligned16(dst, src)) {
    if (nbytes == 0) return;
    hipLaunchKernelGGL(assign_tail_kernel, dim3(CapGrid(GridFor(nbytes), grid_cap)),
                       dim3(kBlock), 0, s, static_cast<char*>(dst),
                       static_cast<const char*>(src), size_t{0}, nbytes);
    return;
  }
  size_t n4 = nbytes / 16;
  if (n4) {
    hipLaunchKernelGGL(assign_kernel, dim3(CapGrid(GridFor(n4), grid_cap)), dim3(kBlock), 0, s,
                       static_cast<uint4*>(dst), static_cast<const uint4*>(src), n4);
  }
  if (nbytes % 16) {
    hipLaunchKernelGGL(assign_tail_kernel, dim3(1), dim3(kBlock), 0, s, static_cast<char*>(dst),
                       static_cast<const char*>(src), n4 * 16, nbytes);
  }
}

void DenseAssign2(void* dst0, void* dst1, const void* src, size_t nbytes, hipStream_t s,
                  int grid_cap) {
  if (nbytes == 0) return;
  // the 16 B path needs all three pointers 16 B-aligned (pool buffers
  // are); anything else takes the byte loop for the whole range
  bool aligned = ((reinterpret_cast<uintptr_t>(dst0) | reinterpret_cast<uintptr_t>(dst1) |
                   reinterpret_cast<uintptr_t>(src)) & 15u) == 0;
  size_t n4 = aligned ? nbytes / 16 : 0;
  int grid = GridFor(n4 ? n4 : nbytes);
  if (grid_cap > 0 && grid > grid_cap) grid = grid_cap;
  hipLaunchKernelGGL(assign2_kernel, dim3(grid), dim3(kBlock), 0, s, static_cast<uint4*>(dst0),
                     static_cast<uint4*>(dst1), static_cast<const uint4*>(src), n4, n4 * 16,
                     nbytes);
}

void DenseSumF32(float* dst, const float* src, size_t n, hipStream_t s, int grid_cap) {
  if (!Aligned16(dst, src)) {
    if (n == 0) return;
    hipLaunchKernelGGL(sum_tail_f32, dim3(CapGrid(GridFor(n), grid_cap)), dim3(kBlock), 0, s, dst,
                       src, size_t{0}, n);
    return;
  }
  size_t n4 = n / 4;
  if (n4) {
    hipLaunchKernelGGL(sum_kernel_f32, dim3(CapGrid(GridFor(n4), grid_cap)), dim3(kBlock), 0, s,
                       reinterpret_cast<float4*>(dst), reinterpret_cast<const float4*>(src), n4);
  }
  if (n % 4) {
    hipLaunchKernelGGL(sum_tail_f32, dim3(1), dim3(kBlock), 0, s, dst, src, n4 * 4, n);
  }
}

void DenseSumBf16(uint16_t* dst, const uint16_t* src, size_t n, hipStream_t s, int grid_cap) {
  if (!Aligned16(dst, src)) {
    if (n == 0) return;
    hipLaunchKernelGGL(sum_tail_bf16, dim3(CapGrid(GridFor(n), grid_cap)), dim3(kBlock), 0, s,
                       dst, src, size_t{0}, n);
    return;
  }
  size_t n8 = n / 8;
  if (n8) {
    hipLaunchKernelGGL(sum_kernel_bf16, dim3(CapGrid(GridFor(n8), grid_cap)), dim3(kBlock), 0, s,
                       reinterpret_cast<uint4*>(dst), reinterpret_cast<const uint4*>(src), n8);
  }
  if (n % 8) {
    hipLaunchKernelGGL(sum_tail_bf16, dim3(1), dim3(kBlock), 0, s, dst, src, n8 * 8, n);
  }
}

void BatchedSumBf16(const CopyDesc* descs_host, int n, hipStream_t s, int tile_cap) {
  if (BalancedBatchEnabled()) {
    LaunchBalanced<2>(descs_host, n, s, tile_cap);
    return;
  }
  LaunchLegacy(batched_sum_kernel_bf16, descs_host, n, s, tile_cap);
}

// the sparse kernels' grid: up to 16384 blocks, fewer under a grid_cap
static int SparseGrid(size_t work_items, int grid_cap) {
  return CapGrid(GridFor(work_items, 16384), grid_cap);
}

void SparseGatherF32(const float* table, const uint64_t* rows_dev, size_t nrows, size_t row_len,
                     float* out, hipStream_t s, int key_shift, uint64_t row_base,
                     uint64_t table_rows, int grid_cap) {
  if (row_len % 4 == 0) {
    hipLaunchKernelGGL(gather_rows_f32, dim3(SparseGrid(nrows * (row_len / 4), grid_cap)),
                       dim3(kBlock), 0, s, reinterpret_cast<const float4*>(table), rows_dev,
                       nrows, row_len / 4, reinterpret_cast<float4*>(out), key_shift, row_base,
                       table_rows);
  } else {
    hipLaunchKernelGGL(gather_rows_scalar_f32, dim3(SparseGrid(nrows * row_len, grid_cap)),
                       dim3(kBlock), 0, s, table, rows_dev, nrows, row_len, out, key_shift,
                       row_base, table_rows);
  }
}

void SparseScatterAssignF32(float* table, const uint64_t* rows_dev, size_t nrows, size_t row_len,
                            const float* src, hipStream_t s, int key_shift, uint64_t row_base,
                            uint64_t table_rows, int grid_cap) {
  if (row_len % 4 == 0) {
    hipLaunchKernelGGL(scatter_assign_rows_f32, dim3(SparseGrid(nrows * (row_len / 4), grid_cap)),
                       dim3(kBlock), 0, s, reinterpret_cast<float4*>(table), rows_dev, nrows,
                       row_len / 4, reinterpret_cast<const float4*>(src), key_shift, row_base,
                       table_rows);
  } else {
    hipLaunchKernelGGL(scatter_assign_rows_scalar_f32,
                       dim3(SparseGrid(nrows * row_len, grid_cap)), dim3(kBlock), 0, s, table,
                       rows_dev, nrows, row_len, src, key_shift, row_base, table_rows);
  }
}

void SparseScatterAddF32(float* table, const uint64_t* rows_dev, size_t nrows, size_t row_len,
                         const float* src, bool atomic, hipStream_t s, int key_shift,
                         uint64_t row_base, uint64_t table_rows, int grid_cap) {
  if (atomic || row_len % 4 != 0) {
    hipLaunchKernelGGL(scatter_add_rows_atomic_f32, dim3(SparseGrid(nrows * row_len, grid_cap)),
                       dim3(kBlock), 0, s, table, rows_dev, nrows, row_len, src, key_shift,
                       row_base, table_rows);
  } else {
    hipLaunchKernelGGL(scatter_add_rows_f32, dim3(SparseGrid(nrows * (row_len / 4), grid_cap)),
                       dim3(kBlock), 0, s, reinterpret_cast<float4*>(table), rows_dev, nrows,
                       row_len / 4, reinterpret_cast<const float4*>(src), key_shift, row_base,
                       table_rows);
  }
}

}  // namespace kern
}  // namespace xps
