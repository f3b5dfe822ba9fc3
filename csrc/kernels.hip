// CDNA4 (gfx950) kernels for the KVServer request handlers.
//
// All kernels are HBM-bandwidth-bound streaming ops, so the design rules
// are (cdna_hip_programming.md §2): 16 B per lane per instruction
// (uint4/float4), 64-wide wavefronts, grid-stride loops sized >> 256
// workgroups to fill 8 XCDs, and a single pass over dst for the
// multi-source reduction. Inputs may be hipIpc-mapped peer-GPU memory —
// the loads then ride xGMI.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "kernels.h"
#include "tile_runs.h"

namespace xps {
namespace kern {

namespace {

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

// The three dense ops, each in its 16 B form (one Vec per lane per step)
// and its element form; every kernel template below takes one of them.

// dst = src, bytes; dst is never loaded
struct CopyOp {
  using Vec = uint4;
  using Elem = char;
  __device__ static void Do(uint4* dst, const uint4* src, size_t i) { dst[i] = src[i]; }
  __device__ static void Do(char* dst, const char* src, size_t i) { dst[i] = src[i]; }
};

// dst += src, fp32
struct SumF32Op {
  using Vec = float4;
  using Elem = float;
  __device__ static void Do(float4* dst, const float4* src, size_t i) {
    float4 d = dst[i];
    float4 s = src[i];
    d.x += s.x;
    d.y += s.y;
    d.z += s.z;
    d.w += s.w;
    dst[i] = d;
  }
  __device__ static void Do(float* dst, const float* src, size_t i) { dst[i] += src[i]; }
};

// dst += src, bf16 with the add in fp32, 8 elements per uint4
struct SumBf16Op {
  using Vec = uint4;
  using Elem = uint16_t;
  __device__ static void Do(uint4* dst, const uint4* src, size_t i) {
    uint4 d = dst[i];
    uint4 s = src[i];
    d.x = bf16x2_sum(d.x, s.x);
    d.y = bf16x2_sum(d.y, s.y);
    d.z = bf16x2_sum(d.z, s.z);
    d.w = bf16x2_sum(d.w, s.w);
    dst[i] = d;
  }
  __device__ static void Do(uint16_t* dst, const uint16_t* src, size_t i) {
    dst[i] = f32_to_bf16(bf16_to_f32(dst[i]) + bf16_to_f32(src[i]));
  }
};

// grid-stride sweep of nvec 16 B vectors
//
// NOTE: nontemporal loads/stores were measured 3 % SLOWER end-to-end
// here, with the push and the pull as two kernels (the pull re-read the
// just-written store). Keep plain float4. For the dual-write kernels
// below, which have no such re-read, the hints were measured again and
// lost again (see batched_assign2_kernel).
template <class Op>
__global__ void dense_kernel(typename Op::Vec* __restrict__ dst,
                             const typename Op::Vec* __restrict__ src, size_t nvec) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < nvec; i += stride) Op::Do(dst, src, i);
}

// The element kernel serves two launches: one block for the sub-16 B tail
// [nvec * 16 B, n) of an aligned range, and a grid-stride sweep of a whole
// range [0, n) whose pointers are not 16 B-aligned.
template <class Op>
__global__ void dense_elem_kernel(typename Op::Elem* __restrict__ dst,
                                  const typename Op::Elem* __restrict__ src, size_t begin,
                                  size_t end) {
  size_t i = begin + blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < end; i += stride) Op::Do(dst, src, i);
}

// Fused push+pull of one key: one 16 B load per lane per iteration, two
// 16 B stores (store entry + the requester's pull destination). Moves
// 3 bytes of traffic per payload byte where a pair of copy kernels moved
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

// balanced variant: segments are concatenated into one virtual chunk
// space (prefix = exclusive 16-B-chunk offsets); each BLOCK owns
// contiguous tiles of that space, so work splits evenly across mixed
// segment sizes (the per-segment grid-stride left small buckets on a
// handful of blocks while every block swept all 64 segment headers).
// Within a tile lanes stay consecutive (coalesced); the tile's segment
// is found once and walked forward.
template <class Op>
__global__ void batched_balanced_kernel(SegTable<CopyDesc> da, size_t chunks_per_block) {
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
    Op::Do(static_cast<typename Op::Vec*>(da.d[seg].dst),
           static_cast<const typename Op::Vec*>(da.d[seg].src), local);
  }
}

// XPS_BALANCED_BATCH=0: every block strides over every segment's 16 B
// chunks (grid sized for the concatenated total, so all segments together
// fill the 8 XCDs); prefix is not read
// (segment loop per block; fine for <= kMaxBatch segments)
template <class Op>
__global__ void batched_legacy_kernel(SegTable<CopyDesc> da) {
  for (int seg = 0; seg < da.n; ++seg) {
    typename Op::Vec* dst = static_cast<typename Op::Vec*>(da.d[seg].dst);
    const typename Op::Vec* src = static_cast<const typename Op::Vec*>(da.d[seg].src);
    size_t nvec = da.d[seg].nbytes / 16;
    size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
    size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (; i < nvec; i += stride) Op::Do(dst, src, i);
  }
}

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
    batched_assign2_kernel(SegTable<Seg2> da, size_t chunks_per_block) {
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

bool BalancedBatchEnabled() {
  static const bool on = [] {
    const char* v = getenv("XPS_BALANCED_BATCH");
    return !v || atoi(v) != 0;  // default on
  }();
  return on;
}

unsigned long long Chunks(const CopyDesc& d) { return d.nbytes / 16; }

template <class Op>
void LaunchBatched(const CopyDesc* descs_host, int n, hipStream_t s, int tile_cap) {
  if (BalancedBatchEnabled()) {
    ForEachTable(descs_host, n, Chunks, [&](const SegTable<CopyDesc>& da, size_t total) {
      // tile size: fill ~8192 blocks (8 XCDs want >> 256 workgroups),
      // whole multiples of the block so lanes sweep full strides (under a
      // tile_cap the tile grows and a block sweeps several strides of it)
      size_t cpb = TileChunks(total, kBlock, 8192, 0, tile_cap);
      hipLaunchKernelGGL(batched_balanced_kernel<Op>, dim3(TileGrid(total, cpb)), dim3(kBlock), 0,
                         s, da, cpb);
    });
    return;
  }
  // one grid for every table, sized for the whole list
  size_t total = 0;
  for (int i = 0; i < n; ++i) total += descs_host[i].nbytes;
  int grid = GridFor(total / 16, 8192, tile_cap);
  ForEachTable(descs_host, n, Chunks, [&](const SegTable<CopyDesc>& da, size_t) {
    hipLaunchKernelGGL(batched_legacy_kernel<Op>, dim3(grid), dim3(kBlock), 0, s, da);
  });
}

// The dense launchers' plan over n elements: the 16 B kernel and one block
// of the element kernel for what is left past the last whole vector, or,
// when a pointer is not 16 B-aligned, the element kernel for the whole range.
template <class Op>
void LaunchDense(typename Op::Elem* dst, const typename Op::Elem* src, size_t n, hipStream_t s,
                 int grid_cap) {
  using Vec = typename Op::Vec;
  constexpr size_t kPerVec = sizeof(Vec) / sizeof(typename Op::Elem);
  if (!Aligned16(dst, src)) {
    if (n == 0) return;
    hipLaunchKernelGGL(dense_elem_kernel<Op>, dim3(GridFor(n, 8192, grid_cap)), dim3(kBlock), 0, s,
                       dst, src, size_t{0}, n);
    return;
  }
  size_t nvec = n / kPerVec;
  if (nvec) {
    hipLaunchKernelGGL(dense_kernel<Op>, dim3(GridFor(nvec, 8192, grid_cap)), dim3(kBlock), 0, s,
                       reinterpret_cast<Vec*>(dst), reinterpret_cast<const Vec*>(src), nvec);
  }
  if (n % kPerVec) {
    hipLaunchKernelGGL(dense_elem_kernel<Op>, dim3(1), dim3(kBlock), 0, s, dst, src,
                       nvec * kPerVec, n);
  }
}

}  // namespace

void BatchedAssign(const CopyDesc* descs_host, int n, hipStream_t s, int tile_cap) {
  LaunchBatched<CopyOp>(descs_host, n, s, tile_cap);
}

void BatchedSumF32(const CopyDesc* descs_host, int n, hipStream_t s, int tile_cap) {
  LaunchBatched<SumF32Op>(descs_host, n, s, tile_cap);
}

void BatchedSumBf16(const CopyDesc* descs_host, int n, hipStream_t s, int tile_cap) {
  LaunchBatched<SumBf16Op>(descs_host, n, s, tile_cap);
}

void BatchedAssign2(const Seg2* segs_host, int n, hipStream_t s, int tile_cap) {
  ForEachTable(
      segs_host, n, [](const Seg2& sg) { return sg.nbytes / 16; },
      [&](const SegTable<Seg2>& da, size_t total) {
        // tile size: whole multiples of the block so lanes sweep full
        // strides, enough for ~8192 blocks on a small launch, and no more
        // than kTileChunks2 however large the launch (past 64 MiB the grid
        // grows instead of the tile). A tile_cap is obeyed as given.
        size_t cpb = TileChunks(total, kBlock, 8192, kTileChunks2, tile_cap);
        hipLaunchKernelGGL(batched_assign2_kernel, dim3(TileGrid(total, cpb)), dim3(kBlock), 0, s,
                           da, cpb);
      });
}

void DenseAssign(void* dst, const void* src, size_t nbytes, hipStream_t s, int grid_cap) {
  LaunchDense<CopyOp>(static_cast<char*>(dst), static_cast<const char*>(src), nbytes, s, grid_cap);
}

void DenseSumF32(float* dst, const float* src, size_t n, hipStream_t s, int grid_cap) {
  LaunchDense<SumF32Op>(dst, src, n, s, grid_cap);
}

void DenseSumBf16(uint16_t* dst, const uint16_t* src, size_t n, hipStream_t s, int grid_cap) {
  LaunchDense<SumBf16Op>(dst, src, n, s, grid_cap);
}

void DenseAssign2(void* dst0, void* dst1, const void* src, size_t nbytes, hipStream_t s,
                  int grid_cap) {
  if (nbytes == 0) return;
  // with a misaligned pointer the byte loop takes the whole range
  size_t n4 = Aligned16(dst0, dst1, src) ? nbytes / 16 : 0;
  int grid = GridFor(n4 ? n4 : nbytes, 8192, grid_cap);
  hipLaunchKernelGGL(assign2_kernel, dim3(grid), dim3(kBlock), 0, s, static_cast<uint4*>(dst0),
                     static_cast<uint4*>(dst1), static_cast<const uint4*>(src), n4, n4 * 16,
                     nbytes);
}

// the sparse kernels' grid: up to 16384 blocks, fewer under a grid_cap
static int SparseGrid(size_t work_items, int grid_cap) {
  return GridFor(work_items, 16384, grid_cap);
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
