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
// Adagrad step on the rows r whose decoded row lies in the table, g = grad[r]
// (sparse_opt.hip):
//   rowwise:      state[row]    += sum(g * g) / row_len  (one float per row)
//   element-wise: state[row][c] += g[c] * g[c]           (the table's shape)
//   table[row][c] -= lr * g[c] / (sqrt(new state) + eps)
// With out_or_null set, out[r] receives the new row, or zeros for a row
// outside the table (what the gather gives); table and state are not
// touched for such a row. In-range rows of one call must be unique, and
// table, state, grad and out pairwise disjoint. Rows move as float4 when
// row_len % 4 == 0 and table, grad, out (and an element-wise state) are
// 16 B-aligned, else as single floats. lr <= 0 or eps <= 0 is
// std::invalid_argument and nothing is launched.
void SparseAdagradF32(float* table, float* state, const uint64_t* rows_dev, size_t nrows,
                      size_t row_len, const float* grad, float* out_or_null, float lr, float eps,
                      bool rowwise, hipStream_t s, int key_shift = 0, uint64_t row_base = 0,
                      uint64_t table_rows = ~0ull, int grid_cap = 0);
// Sparse ("lazy") Adam step on the rows r whose decoded row lies in the
// table, g = grad[r] (sparse_opt.hip). The bias correction is the row's own:
// p1, p2 are the running products beta1^t, beta2^t of that row's steps.
//   p1' = p1 * beta1,  p2' = p2 * beta2
//   m'  = beta1 * m + (1 - beta1) * g
//   v'  = beta2 * v + (1 - beta2) * g * g                 (element-wise)
//   v'  = beta2 * v + (1 - beta2) * sum(g * g) / row_len  (rowwise: one float per row)
//   w'  = w - (lr / (1 - p1')) * m' / (sqrt(v' / (1 - p2')) + eps)
// state holds one record per table row,
//   { p1, p2, v_row, 0 }  m[row_len]  v[row_len] (element-wise only)
// SparseLazyAdamStateFloats floats in all; a fresh state has p1 = p2 = 1 and
// +0.0 everywhere else (v_row is unused element-wise). out_or_null, row
// uniqueness, disjointness and rows outside the table are as for Adagrad.
// Rows move as float4 when row_len % 4 == 0 and table, grad and out are
// 16 B-aligned, else as single floats. lr <= 0, eps <= 0, a beta outside
// [0, 1) or a state off a 16 B boundary is std::invalid_argument and nothing
// is launched.
size_t SparseLazyAdamStateFloats(size_t rows, size_t row_len, bool rowwise);
void SparseLazyAdamF32(float* table, float* state, const uint64_t* rows_dev, size_t nrows,
                       size_t row_len, const float* grad, float* out_or_null, float lr, float beta1,
                       float beta2, float eps, bool rowwise, hipStream_t s, int key_shift = 0,
                       uint64_t row_base = 0, uint64_t table_rows = ~0ull, int grid_cap = 0);
// The same ops over a bf16 table (sparse_bf16.hip): `table` holds bf16 bits,
// every other array stays fp32. A weight is widened exactly, the fp32
// operations are those of the F32 sibling in the same order, and the result
// x (bits u) is rounded once on the store by R:
//   kNearest:    round-to-nearest-even
//   kStochastic: (u + r) >> 16, r uniform in [0, 2^16): the magnitude goes up
//                with probability (u & 0xffff) / 2^16; a bf16 value keeps its bits
// Inf and NaN pass through both. r is 16 bits of a counter-based generator
// keyed on (seed, local row, element index) (SplitMix64, stated at the top
// of sparse_bf16.hip): the same call gives the same table bits under any
// grid_cap and on either path. Rows move as 8-element units (one 16 B table
// access against two float4) when row_len % 8 == 0 and the table and the
// fp32 arrays (an element-wise Adagrad state included) are 16 B-aligned,
// else element by element for the whole call.
enum class Bf16Rounding { kNearest, kStochastic };
// the seed of a handler's n-th rounding launch: mix(seed + (n + 1) * phi)
uint64_t SparseBf16LaunchSeed(uint64_t seed, uint64_t n);
// out[r][:] = float(table[row(r)][:]), exact; zeros for a key outside the table
void SparseGatherBf16(const uint16_t* table, const uint64_t* rows_dev, size_t nrows,
                      size_t row_len, float* out, hipStream_t s, int key_shift = 0,
                      uint64_t row_base = 0, uint64_t table_rows = ~0ull, int grid_cap = 0);
// table[row(r)][:] = RNE_bf16(src[r][:]): always nearest, no seed (how
// weights are initialised)
void SparseScatterAssignBf16(uint16_t* table, const uint64_t* rows_dev, size_t nrows,
                             size_t row_len, const float* src, hipStream_t s, int key_shift = 0,
                             uint64_t row_base = 0, uint64_t table_rows = ~0ull,
                             int grid_cap = 0);
// table[row(r)][:] = R(float(table[row(r)][:]) + src[r][:]), one fp32 add.
// Not atomic: in-range rows of one call must be unique, and calls on one
// table ordered by the caller.
void SparseScatterAddBf16(uint16_t* table, const uint64_t* rows_dev, size_t nrows, size_t row_len,
                          const float* src, Bf16Rounding rounding, uint64_t seed, hipStream_t s,
                          int key_shift = 0, uint64_t row_base = 0, uint64_t table_rows = ~0ull,
                          int grid_cap = 0);
// SparseAdagradF32 / SparseLazyAdamF32 with table[row][c] = R(w'): the same
// state layouts, records, requirements and std::invalid_argument cases. With
// out_or_null set, out[r][c] is the stored bf16 widened, what a later gather
// returns bit for bit (not the unrounded w'), or zeros for a row outside the
// table.
void SparseAdagradBf16(uint16_t* table, float* state, const uint64_t* rows_dev, size_t nrows,
                       size_t row_len, const float* grad, float* out_or_null, float lr, float eps,
                       bool rowwise, Bf16Rounding rounding, uint64_t seed, hipStream_t s,
                       int key_shift = 0, uint64_t row_base = 0, uint64_t table_rows = ~0ull,
                       int grid_cap = 0);
void SparseLazyAdamBf16(uint16_t* table, float* state, const uint64_t* rows_dev, size_t nrows,
                        size_t row_len, const float* grad, float* out_or_null, float lr,
                        float beta1, float beta2, float eps, bool rowwise, Bf16Rounding rounding,
                        uint64_t seed, hipStream_t s, int key_shift = 0, uint64_t row_base = 0,
                        uint64_t table_rows = ~0ull, int grid_cap = 0);
// The bf16-table ops with bf16 bits on the wire side too: gradients and
// pushed values come as bf16 bits and are widened exactly, rows out are the
// stored bits (0x0000 for a key outside the table). Fed bits b, a step or an
// add leaves the table and state bits its sibling above leaves fed widen(b).
// 8-element units (one 16 B access per array) need row_len % 8 == 0 and
// table, grad/src and out (and an element-wise Adagrad state) 16 B-aligned;
// else the whole call moves uint16_t against uint16_t. Everything else,
// the std::invalid_argument cases included, is the sibling's.
// out[r][:] = table[row(r)][:] as bits
void SparseGatherBf16Wire(const uint16_t* table, const uint64_t* rows_dev, size_t nrows,
                          size_t row_len, uint16_t* out, hipStream_t s, int key_shift = 0,
                          uint64_t row_base = 0, uint64_t table_rows = ~0ull, int grid_cap = 0);
// table[row(r)][:] = src[r][:] as bits: no rounding, the sender rounded
void SparseScatterAssignBf16Wire(uint16_t* table, const uint64_t* rows_dev, size_t nrows,
                                 size_t row_len, const uint16_t* src, hipStream_t s,
                                 int key_shift = 0, uint64_t row_base = 0,
                                 uint64_t table_rows = ~0ull, int grid_cap = 0);
// table[row(r)][c] = R(float(table[row(r)][c]) + float(src[r][c])), one fp32 add
void SparseScatterAddBf16Wire(uint16_t* table, const uint64_t* rows_dev, size_t nrows,
                              size_t row_len, const uint16_t* src, Bf16Rounding rounding,
                              uint64_t seed, hipStream_t s, int key_shift = 0,
                              uint64_t row_base = 0, uint64_t table_rows = ~0ull,
                              int grid_cap = 0);
// SparseAdagradBf16 with g = float(grad bits); out[r][c] = the stored bits
void SparseAdagradBf16Wire(uint16_t* table, float* state, const uint64_t* rows_dev, size_t nrows,
                           size_t row_len, const uint16_t* grad, uint16_t* out_or_null, float lr,
                           float eps, bool rowwise, Bf16Rounding rounding, uint64_t seed,
                           hipStream_t s, int key_shift = 0, uint64_t row_base = 0,
                           uint64_t table_rows = ~0ull, int grid_cap = 0);
// SparseLazyAdamBf16 with g = float(grad bits); out[r][c] = the stored bits
void SparseLazyAdamBf16Wire(uint16_t* table, float* state, const uint64_t* rows_dev, size_t nrows,
                            size_t row_len, const uint16_t* grad, uint16_t* out_or_null, float lr,
                            float beta1, float beta2, float eps, bool rowwise,
                            Bf16Rounding rounding, uint64_t seed, hipStream_t s, int key_shift = 0,
                            uint64_t row_base = 0, uint64_t table_rows = ~0ull, int grid_cap = 0);
// Worker side of the sparse ops (sparse_coalesce.hip): a batch's ids, in any
// order and with any repetition, become the sorted unique keys the ops above
// and the handlers want. ids compare as unsigned 64-bit values.
//   uniq_keys[0, m): the distinct ids, strictly ascending, each << key_shift
//   inverse[i]:      the slot in [0, m) of ids[i], for every i < n
//   sums[u]:         +0.0, then + grad[i] for every i < grad_rows with
//                    inverse[i] == u, in ascending i, one IEEE fp32 add each
//                    (np.add.at on a zero array, bit for bit); occurrences
//                    i >= grad_rows name a row without a gradient
// Returns m after synchronising s. uniq_keys and inverse have n slots, sums
// n x row_len (rows past m are not written); grad_or_null = null gives rows
// of +0.0, sums_or_null = null skips the sums. Rows move as float4 when
// row_len % 4 == 0 and grad and sums are 16 B-aligned, else as floats.
// n == 0 returns 0 without a HIP call. std::invalid_argument before any HIP
// call: n >= 2^31, grad_rows > n, a gradient with row_len == 0, a workspace
// below SparseCoalesceWorkspaceBytes(n), key_shift outside [0, 63], and
// ids, uniq_keys or inverse off an 8 B boundary.
// Limit: one group of lanes sums a whole segment, so one very hot id in a
// huge batch serialises; splitting a segment would change the add order.
int SparseCoalesceTile();  // elements a block sorts in LDS
size_t SparseCoalesceWorkspaceBytes(size_t n);
size_t SparseCoalesce(const uint64_t* ids_dev, size_t n, int key_shift, const float* grad_or_null,
                      size_t grad_rows, size_t row_len, uint64_t* uniq_keys, float* sums_or_null,
                      int64_t* inverse, void* workspace, size_t workspace_bytes, hipStream_t s,
                      int grid_cap = 0);
// SparseCoalesce with the sums as bf16 bits, what a 16-bit wire pushes: each
// fp32 sum as above, rounded once to nearest even on the store. 8 sums move
// as one 16 B store when row_len % 8 == 0 and grad and sums are 16 B-aligned.
size_t SparseCoalesceBf16(const uint64_t* ids_dev, size_t n, int key_shift,
                          const float* grad_or_null, size_t grad_rows, size_t row_len,
                          uint64_t* uniq_keys, uint16_t* sums_or_null, int64_t* inverse,
                          void* workspace, size_t workspace_bytes, hipStream_t s,
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
