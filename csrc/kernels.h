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
// Sparse ops over an embedding table (sparse_table.hip; the fp32 table's
// gather, assign and add kernels are kernels.hip's). A call names its rows
// (SparseRows), its table (SparseTable) and its wire side, the gradients or
// pushed values in and the rows out (SparseWire); the dtypes are dispatched
// inside the five entry points. An fp32 table with a bf16 wire, and an atomic
// add on a bf16 table, have no kernel: std::invalid_argument before any HIP
// call, like every argument check below.
enum class SparseDtype { kF32, kBf16 };
// Which rows a call touches and where it runs. Local row index =
// (keys[r] >> key_shift) - row_base, so a server can index its local table
// shard from globally-sharded keys (key = global_row << key_shift spreads
// rows over the PS key space). table_rows bounds every decoded row index:
// out-of-range rows (corrupt or misrouted keys) are skipped by scatters and
// steps and read as zeros by gathers, never touching memory outside the
// table. The ~0 default disables the check (trusted keys). grid_cap > 0 caps
// the grid (tests).
struct SparseRows {
  const uint64_t* keys;  // device memory
  size_t nrows;
  size_t row_len;
  int key_shift = 0;
  uint64_t row_base = 0;
  uint64_t table_rows = ~0ull;
  hipStream_t s = nullptr;
  int grid_cap = 0;
};
// A bf16 table holds bf16 bits and says how a result x (bits u) is rounded
// on the store, the rule R:
//   kNearest:    round-to-nearest-even
//   kStochastic: (u + r) >> 16, r uniform in [0, 2^16): the magnitude goes up
//                with probability (u & 0xffff) / 2^16; a bf16 value keeps its bits
// Inf and NaN pass through both. r is 16 bits of a counter-based generator
// keyed on (seed, local row, element index) (SplitMix64, stated at the top
// of sparse_table.hip): the same call gives the same table bits under any
// grid_cap and on either path. An fp32 table stores x itself and ignores
// rounding and seed.
enum class Bf16Rounding { kNearest, kStochastic };
struct SparseTable {
  void* p;
  SparseDtype dtype;
  Bf16Rounding rounding = Bf16Rounding::kNearest;
  uint64_t seed = 0;
};
// fp32 values, or for a bf16 table bf16 bits: values in are widened exactly,
// rows out are the stored bits (0x0000 for a key outside the table). Fed bits
// b, a step or an add leaves the table and state bits it leaves fed widen(b)
// on the fp32 wire.
struct SparseWire {
  void* p;
  SparseDtype dtype;
};
// the seed of a handler's n-th rounding launch: mix(seed + (n + 1) * phi)
uint64_t SparseBf16LaunchSeed(uint64_t seed, uint64_t n);
// How rows move. An fp32 table: as float4 when row_len % 4 == 0 (gather,
// assign, add), for a step when also table, grad and out (and an
// element-wise Adagrad state) are 16 B-aligned, else as single floats. A
// bf16 table: as 8-element units (one 16 B table access against two float4,
// or against one 16 B access of a bf16 wire) when row_len % 8 == 0 and the
// table and the wire arrays (and an element-wise Adagrad state) are
// 16 B-aligned, else element by element for the whole call.
//
// out[r][:] = table[row(r)][:] for r in [0, nrows), a bf16 weight widened
// exactly (bf16 wire: as bits); zeros for a key outside the table
void SparseGather(const SparseTable& table, const SparseRows& rows, SparseWire out);
// table[row(r)][:] = src[r][:]. A bf16 table stores RNE_bf16(src): always
// nearest, no seed (how weights are initialised); from a bf16 wire the bits
// as they are, the sender rounded.
void SparseScatterAssign(const SparseTable& table, const SparseRows& rows, SparseWire src);
// table[row(r)][:] = R(table[row(r)][:] + src[r][:]), one fp32 add.
// atomic = true (fp32 table only) tolerates duplicate rows; otherwise
// in-range rows of one call must be unique, and calls on one table ordered by
// the caller.
void SparseScatterAdd(const SparseTable& table, const SparseRows& rows, SparseWire src,
                      bool atomic = false);
// Adagrad step on the rows r whose decoded row lies in the table, g = grad[r]:
//   rowwise:      state[row]    += sum(g * g) / row_len  (one float per row)
//   element-wise: state[row][c] += g[c] * g[c]           (the table's shape)
//   table[row][c] = R(table[row][c] - lr * g[c] / (sqrt(new state) + eps))
// The state is fp32 whatever the table; a bf16 weight is widened exactly, the
// fp32 operations are the fp32 table's in the same order, and the result is
// rounded once on the store. With out_or_null.p set, out[r] receives the new
// row as stored, what a later gather returns bit for bit (not the unrounded
// w'), or zeros for a row outside the table; table and state are not touched
// for such a row. out is of grad's dtype. In-range rows of one call must be
// unique, and table, state, grad and out pairwise disjoint. lr <= 0 or
// eps <= 0 is std::invalid_argument and nothing is launched.
struct AdagradParams {
  float lr;
  float eps;
  bool rowwise;
};
void SparseAdagrad(const SparseTable& table, float* state, const SparseRows& rows,
                   SparseWire grad, SparseWire out_or_null, const AdagradParams& params);
// Sparse ("lazy") Adam step on the rows r whose decoded row lies in the
// table, g = grad[r]. The bias correction is the row's own: p1, p2 are the
// running products beta1^t, beta2^t of that row's steps.
//   p1' = p1 * beta1,  p2' = p2 * beta2
//   m'  = beta1 * m + (1 - beta1) * g
//   v'  = beta2 * v + (1 - beta2) * g * g                 (element-wise)
//   v'  = beta2 * v + (1 - beta2) * sum(g * g) / row_len  (rowwise: one float per row)
//   w'  = R(w - (lr / (1 - p1')) * m' / (sqrt(v' / (1 - p2')) + eps))
// state holds one record per table row,
//   { p1, p2, v_row, 0 }  m[row_len]  v[row_len] (element-wise only)
// SparseLazyAdamStateFloats floats in all; a fresh state has p1 = p2 = 1 and
// +0.0 everywhere else (v_row is unused element-wise). The table's dtype,
// out_or_null, row uniqueness, disjointness and rows outside the table are as
// for Adagrad. lr <= 0, eps <= 0, a beta outside [0, 1) or a state off a
// 16 B boundary is std::invalid_argument and nothing is launched.
struct LazyAdamParams {
  float lr;
  float beta1, beta2;
  float eps;
  bool rowwise;
};
size_t SparseLazyAdamStateFloats(size_t rows, size_t row_len, bool rowwise);
void SparseLazyAdam(const SparseTable& table, float* state, const SparseRows& rows,
                    SparseWire grad, SparseWire out_or_null, const LazyAdamParams& params);
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
