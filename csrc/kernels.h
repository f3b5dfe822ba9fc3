// Host-side launchers for the CDNA4 server kernels (kernels.hip).
//
// These implement the compute the ps-lite server handler API implies
// (dense accumulate/assign replacing KVServerDefaultHandle
// kv_app.h:441-448, sparse gather/scatter over a key-indexed table) —
// all-new HIP code, the reference has no kernels.
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "coalesce_admit.h"
#include "kernel_util.h"

namespace xps {
namespace kern {

// dst[i] = src[i] (bytes; 16B-vectorized grid-stride copy kernel).
// DenseAssign, DenseSumF32 and DenseSumBf16 take the 16 B kernel when dst
// and src are both 16 B-aligned (pool buffers are) and an element-wise
// grid-stride kernel for the whole range when either is not. grid_cap > 0
// caps the grid (tests use it to force many grid-stride iterations on a
// small buffer); 0 leaves the launch as it is.
void DenseAssign(void* dst, const void* src, size_t nbytes, hipStream_t s, int grid_cap = 0);
// dst0[i] = dst1[i] = src[i] (bytes; one 16 B load, two 16 B stores per
// lane — the fused push+pull of one key). The three ranges must be
// pairwise disjoint. grid_cap > 0 caps the grid (tests use it to force
// many grid-stride iterations on a small buffer).
void DenseAssign2(void* dst0, void* dst1, const void* src, size_t nbytes, hipStream_t s,
                  int grid_cap = 0);
// true iff the three len-byte ranges are pairwise disjoint (DenseAssign2's
// precondition; callers check it before choosing the fused kernel)
inline bool Disjoint3(const void* a, const void* b, const void* c, size_t len) {
  auto apart = [len](const void* x, const void* y) {
    uintptr_t p = reinterpret_cast<uintptr_t>(x), q = reinterpret_cast<uintptr_t>(y);
    return p + len <= q || q + len <= p;
  };
  return apart(a, b) && apart(a, c) && apart(b, c);
}
// dst[i] += src[i] (fp32)
void DenseSumF32(float* dst, const float* src, size_t n, hipStream_t s, int grid_cap = 0);
// dst[i] += src[i] (bf16 payloads, fp32 accumulate in-register,
// round-to-nearest-even back to bf16 — halves bytes moved on the
// bandwidth-bound dense path)
void DenseSumBf16(uint16_t* dst, const uint16_t* src, size_t n, hipStream_t s, int grid_cap = 0);
void BatchedSumBf16(const struct CopyDesc* descs_host, int n, hipStream_t s, int tile_cap = 0);
// Sparse ops: local row index = (rows[r] >> key_shift) - row_base, so a
// server can index its local table shard from globally-sharded keys
// (key = global_row << key_shift spreads rows over the PS key space).
// table_rows bounds every decoded row index: out-of-range rows (corrupt
// or misrouted keys) are skipped by scatters and read as zeros by
// gathers, never touching memory outside the table. The ~0 default
// disables the check (trusted keys). grid_cap > 0 caps the grid (tests).
// out[r][:] = table[row(r)][:] for r in [0, nrows)
void SparseGatherF32(const float* table, const uint64_t* rows_dev, size_t nrows, size_t row_len,
                     float* out, hipStream_t s, int key_shift = 0, uint64_t row_base = 0,
                     uint64_t table_rows = ~0ull, int grid_cap = 0);
// table[row(r)][:] += src[r][:]; atomic=true tolerates duplicate rows
void SparseScatterAddF32(float* table, const uint64_t* rows_dev, size_t nrows, size_t row_len,
                         const float* src, bool atomic, hipStream_t s, int key_shift = 0,
                         uint64_t row_base = 0, uint64_t table_rows = ~0ull, int grid_cap = 0);
// table[row(r)][:] = src[r][:]
void SparseScatterAssignF32(float* table, const uint64_t* rows_dev, size_t nrows, size_t row_len,
                            const float* src, hipStream_t s, int key_shift = 0,
                            uint64_t row_base = 0, uint64_t table_rows = ~0ull,
                            int grid_cap = 0);

// Batched segmented copy/accumulate: one launch serving up to
// kMaxBatch (dst, src, nbytes) segments — the device-side slicing/merge
// of SURVEY.md §2.6 item 3, used for multi-key messages.
struct CopyDesc {
  void* dst;
  const void* src;
  size_t nbytes;  // must be 16B-multiples for the batched kernels
};
// The batched kernels' contract for a segment list: every dst and src
// 16 B-aligned, every length a 16 B multiple. A list that fails it goes
// through the per-segment launchers, which take any skew.
inline bool BatchAligned(const CopyDesc* descs, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    if (!Aligned16(descs[i].dst, descs[i].src) || descs[i].nbytes % 16) return false;
  }
  return true;
}
// Segments may be empty. tile_cap > 0 caps the number of blocks (tests):
// on the balanced path the tile grows and a block sweeps several strides
// of it, on the XPS_BALANCED_BATCH=0 path the grid-stride grid shrinks.
void BatchedAssign(const CopyDesc* descs_host, int n, hipStream_t s, int tile_cap = 0);
void BatchedSumF32(const CopyDesc* descs_host, int n, hipStream_t s, int tile_cap = 0);

// Batched dual write: dst0[i] = dst1[i] = src[i] for every segment, in
// one launch per kMaxBatch segments (the coalesced form of DenseAssign2:
// keys queued behind a busy GPU share one launch). Every segment needs
// its three pointers 16 B-aligned, nbytes % 16 == 0 and pairwise-disjoint
// ranges; segments of one call must not conflict with each other
// (CoalesceAdmit). tile_cap > 0 caps the grid (tests use it to force
// several tile iterations per block on small inputs).
static_assert(kMaxBatch2 == kMaxBatch, "Seg2 batches use the batched kernels' segment limit");
void BatchedAssign2(const Seg2* segs_host, int n, hipStream_t s, int tile_cap = 0);

// MXFP8 payloads (mxfp8.h: 512 fp32 elements per 528-byte superblock, one
// E8M0 scale byte per 32 elements, OCP e4m3fn codes; kernels in mxfp8.hip).
// Every packed pointer must be 16 B-aligned and every packed length a
// multiple of 528, else std::invalid_argument and nothing is launched.
// fp32 pointers may sit at any 4-byte offset; off a 16 B boundary they are
// read and written element-wise. grid_cap / tile_cap > 0 cap the grid
// (tests).
// packed = Q(src[0, n)): any n, writes MxPackedBytes(n) bytes, the last
// superblock zero-filled past n
void MxQuantize(const float* src, size_t n, void* packed, hipStream_t s, int grid_cap = 0);
// dst[0, n) = D(packed) * alpha: writes exactly n floats
void MxDequantize(const void* packed, size_t n, float* dst, float alpha, hipStream_t s,
                  int grid_cap = 0);
// acc (= | +=) D(packed), one IEEE add per element; acc holds
// nbytes / 528 * 512 floats
void MxAccumulate(float* acc, const void* packed, size_t nbytes, bool assign, hipStream_t s,
                  int grid_cap = 0);
// packed_out = Q((acc or 0) + D(packed_in)); acc is only read
void MxFinish(const float* acc_or_null, const void* packed_in, void* packed_out, size_t nbytes,
              hipStream_t s, int grid_cap = 0);
// The same over segments, one launch per kMaxBatch of them; segments may
// be empty and must not overlap each other. Accumulate ignores out, finish
// takes a null acc as zeros. Both return the number of launches.
struct MxSeg {
  float* acc;
  const void* in;
  void* out;
  size_t nbytes;  // packed bytes of in (and out)
};
int BatchedMxAccumulate(const MxSeg* segs_host, int n, bool assign, hipStream_t s,
                        int tile_cap = 0);
int BatchedMxFinish(const MxSeg* segs_host, int n, hipStream_t s, int tile_cap = 0);
// Worker side over segments, one launch per kMaxBatch non-empty ones;
// output bytes are those of MxQuantize / MxDequantize run per segment.
// Segments must not overlap each other. A launch moves fp32 as float4 when
// every segment in it has a 16 B-aligned f32, else element-wise. A null f32
// on a non-empty segment is std::invalid_argument; a list without a
// non-empty segment makes no HIP call. Both return the number of launches.
struct MxWorkSeg {
  float* f32;    // quantize reads it, dequantize writes it; any 4-byte offset
  void* packed;  // 16 B-aligned; MxPackedBytes(n) bytes
  size_t n;      // elements; any value, 0 = empty segment
};
// packed = Q(f32[0, n)) per segment, the last superblock zero-filled past n
int BatchedMxQuantize(const MxWorkSeg* segs_host, int n, hipStream_t s, int tile_cap = 0);
// f32[0, n) = D(packed) * alpha per segment: exactly n floats written
int BatchedMxDequantize(const MxWorkSeg* segs_host, int n, float alpha, hipStream_t s,
                        int tile_cap = 0);

}  // namespace kern
}  // namespace xps
