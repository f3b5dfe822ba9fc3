// Built-in GPU request handlers for KVServer<float>.
//
// Reference parity: ps-lite ships only CPU handlers — the tests'
// EmptyHandler (tests/test_benchmark.cc:132-203, stores pushed buffers,
// echoes on pull) and KVServerDefaultHandle (kv_app.h:431-452,
// store[key] += vals). Here both behaviors are CDNA4 kernels on the
// requester's per-peer HIP stream: push = DenseAssign / DenseSumF32
// reading the worker's HBM directly (hipIpc-mapped, reads ride xGMI);
// pull = zero-copy store view handed to the plane's in-place xGMI write.
// The sparse handler owns a rows x row_len fp32 embedding table and uses
// the gather/scatter kernels (BASELINE config #5).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <memory>
#include <set>
#include <type_traits>
#include <unordered_map>

#include "kernels.h"
#include "kv_app.h"

namespace xps {

// A pooled hipEvent_t with shared ownership: freed back to the plane's
// event pool (or destroyed) when the last reference drops. Shared
// ownership lets one recorded event serve as the ordering point for
// every key touched by a batched kernel.
using EventRef = std::shared_ptr<std::remove_pointer<hipEvent_t>::type>;

// handler modes
enum class DenseMode {
  kAssign,  // push overwrites the store (EmptyHandler / pure-goodput)
  kSum,     // push accumulates forever (KVServerDefaultHandle)
  kReduce,  // BytePS round semantics: first push of a round assigns, the
            // rest accumulate; pulls are HELD until all num_workers
            // pushes of the round arrived (cross-stream ordered via
            // events), and the round resets after num_workers pulls.
};

// payload dtype of the accumulate kernels (the wire/pools are bytes;
// bf16 halves bytes moved on the bandwidth-bound dense path). Assign
// mode is dtype-agnostic byte copies either way. kMxfp8 (mxfp8.h) exists
// in reduce mode only: workers push and pull packed superblocks, the round
// accumulates in fp32 and is rounded once more when it closes.
enum class DenseDtype { kF32, kBf16, kMxfp8 };

// launches of the MXFP8 accumulate / finish kernels by reduce-mode pushes
extern std::atomic<uint64_t> g_mx_launches;

class GpuDenseHandler {
 public:
  GpuDenseHandler(Postoffice* po, DenseMode mode, DenseDtype dtype = DenseDtype::kF32);
  ~GpuDenseHandler();
  void operator()(const KVMeta& req, const KVPairs<float>& kvs, KVServer<float>* server);

  // checkpoint / resume of the server KV state (an aux subsystem the
  // reference lacks entirely — SURVEY.md §5.4)
  void Save(const std::string& path);
  void Load(const std::string& path);

  // RegisterRecvBufferWithRank parity (reference kv_app.h:488): make an
  // APP-owned device buffer this key's store entry — pushes land
  // straight in it (zero-copy into user memory), pulls serve from it.
  // The buffer must outlive the handler; if it is pool-resident (e.g.
  // a torch-allocator tensor) the one-sided steady state applies too.
  void RegisterEntry(Key key, void* ptr, size_t nbytes, int device);

 private:
  struct Entry {
    SArray<char> buf;
    // last kernel that touched buf, on WHICHEVER peer stream: with >1
    // workers, concurrent senders use different streams, so every
    // kernel touching this entry waits on last_ev and publishes a new
    // one — otherwise two senders' sum kernels race (lost updates) and
    // a pull can read a half-written store
    EventRef last_ev;
    // superseded (smaller) buffers, kept alive forever: workers may
    // still hold their offsets in one-sided entry caches; stale writes
    // must hit dead-but-owned memory. Workers drop an advert when they
    // send the key in a multi-key push or at another length (KVWorker::
    // Send), so such a write needs a push that raced the replacing one.
    std::vector<SArray<char>> retired;
    // kMxfp8: the round's fp32 accumulator, 2048 bytes per superblock of
    // buf, allocated by the first push that needs it; not checkpointed
    SArray<char> acc;
  };

  // Reduce-mode round state, per KEY-SET: a worker's buckets for this
  // server ride ONE multi-key message per round (BytePS bucketed
  // DenseReduce — collapses 2x169 per-key messages/step to 2 per
  // server), so round accounting is per key-set with one batched
  // sum/assign kernel chain and one event per push. Single-key messages
  // are just groups of size 1. CONTRACT: all workers must use the same
  // key->message grouping (the BytePS layout guarantees it); a key must
  // not appear in two different groups.
  struct Group {
    std::vector<Key> keys;
    std::vector<Entry*> ents;   // store_ entries (node-stable pointers)
    std::vector<size_t> lens;   // byte length per key (set by first push)
    int pushes = 0;
    int pulls = 0;
    std::vector<KVMeta> waiting_pulls;
    // pushes of the NEXT round arriving before this round's pulls drain
    // (KVPairs holds the remote buffer alive until we process + ack)
    std::vector<std::pair<KVMeta, KVPairs<float>>> waiting_pushes;
    // pulls from senders that already pulled this round (next-round pulls)
    std::vector<KVMeta> waiting_next_pulls;
    std::set<int> pulled_senders;
    std::vector<EventRef> round_events;  // one per pusher stream
    std::vector<EventRef> pull_guard;    // pull copies the next round must wait on
    EventRef last_ev;                    // last kernel touching the group
  };

  void HandlePush(const KVMeta& req, const KVPairs<float>& kvs, KVServer<float>* server,
                  bool respond = true);
  // fused push+pull of one key in one dual-write launch (assign mode);
  // false = preconditions not met, nothing done
  bool TryFusedAssign(const KVMeta& req, const KVPairs<float>& kvs, KVServer<float>* server);
  void HandleReducePush(const KVMeta& req, const KVPairs<float>& kvs, KVServer<float>* server);
  // kMxfp8: this push's accumulate or finish launches for the whole key-set
  void ReducePushMx(Group* g, const KVPairs<float>& kvs, hipStream_t stream);
  // count the push, publish its event, ack, release the round's held pulls
  void FinishReducePush(const KVMeta& req, Group* g, KVServer<float>* server,
                        hipStream_t stream);
  void HandlePull(const KVMeta& req, const KVPairs<float>& kvs, KVServer<float>* server);
  void RespondPull(const KVMeta& req, Group* g, KVServer<float>* server);
  // multi-key pull copied straight into the requester's advertised HBM
  // destination, meta-only response; false = not possible, nothing done
  bool TryPullInPlace(const KVMeta& req, const KVPairs<float>& res,
                      std::vector<kern::CopyDesc>* descs, hipStream_t stream,
                      KVServer<float>* server);
  Group* GroupFor(const SArray<Key>& keys);  // find-or-create round group
  hipStream_t Stream(int sender);      // lane 0: push/accumulate kernels
  hipStream_t PullStream(int sender);  // pull lane: response copies
  // same-key event chaining needed for this sender? (>1 workers, or the
  // peer's lanes actually split = cross-device)
  bool NeedChain(int sender);
  void OrderAfter(Entry* e, hipStream_t s);  // wait the entry's last_ev
  // find or create the key's entry; a too-small one gets a zeroed buffer
  // of exactly len bytes and its old one is retired, never freed.
  // EntryFor takes mu_, EntryLocked wants it held.
  Entry* EntryFor(Key key, size_t len);
  Entry* EntryLocked(Key key, size_t len);
  static void GrowReduce(Entry* e, size_t len);  // reduce mode: plain reallocation

  // dtype-dispatched accumulate (nbytes, not elements)
  void SumKernel(void* dst, const void* src, size_t nbytes, hipStream_t s);
  void BatchedSum(const kern::CopyDesc* descs, int n, hipStream_t s);
  // BatchedSum, or SumKernel per segment when the list is off the 16 B grid
  void SumSegments(const std::vector<kern::CopyDesc>& descs, hipStream_t s);

  Postoffice* po_;
  DenseMode mode_;
  DenseDtype dtype_;
  int num_workers_ = 1;
  bool chain_ = false;  // >1 workers: cross-stream same-key ordering needed
  std::mutex mu_;
  std::unordered_map<Key, Entry> store_;
  std::unordered_map<uint64_t, Group> groups_;  // keyset-hash -> round group
  hipStream_t fallback_stream_ = nullptr;
};

// NOTE on key uniqueness: a single sparse push message must not repeat a
// row (ps-lite's sorted-unique key contract); duplicate rows across
// MESSAGES are fine (atomic scatters with >1 workers; handler-serialized
// otherwise).
//
// With an optimizer the handler keeps the optimizer state beside the table
// and the push's cmd names the operation: kCmdDefault = one gradient step
// (kern::SparseAdagrad or kern::SparseLazyAdam; state updated),
// kCmdAssign = assign rows (how weights are initialised; state untouched),
// kCmdSum = add (state untouched). `accumulate` plays no part then.
//
// A bf16 table (SparseTableDtype::kBf16; needs an optimizer) holds
// rows * row_len * 2 bytes and goes through kern::Sparse*Bf16. By default
// the wire does not change: pushes and pull responses stay fp32. With
// wire_dtype kBf16 (needs a bf16 table and an even row_len) every pushed
// value and every pulled row is bf16 bits, through a bf16 kern::SparseWire:
// a row is row_len / 2 of the floats that lens and vals.size() count, a pull
// is exact, and a step leaves the bits the fp32 wire leaves for the same
// gradient values. Nothing of it is checkpointed. The
// n-th launch that rounds (a step or an add; n counts from 0 and is
// checkpointed) gets kern::SparseBf16LaunchSeed(seed, n), so a replayed
// message sequence reproduces the table bit for bit. Without an optimizer
// concurrent workers would need a 16-bit atomic add, which does not exist;
// the optimizer handler orders whole kernels instead (chain_).
enum class SparseOpt { kNone, kAdagrad, kRowwiseAdagrad, kLazyAdam, kRowwiseLazyAdam };
enum class SparseTableDtype { kF32, kBf16 };

struct SparseOptConfig {
  SparseOpt kind = SparseOpt::kNone;
  float lr = 0.01f;
  float eps = 1e-8f;
  float init_acc = 0.f;  // Adagrad: the state's value before the first step
  float beta1 = 0.9f;    // lazy Adam: decay of the first moment
  float beta2 = 0.999f;  // lazy Adam: decay of the second moment
  SparseTableDtype table_dtype = SparseTableDtype::kF32;
  kern::Bf16Rounding rounding = kern::Bf16Rounding::kStochastic;  // bf16 table: the store rule
  uint64_t seed = 0;                                              // bf16 table, stochastic
  SparseTableDtype wire_dtype = SparseTableDtype::kF32;  // what pushes and pulls carry
};

class GpuSparseHandler {
 public:
  // Allocates (and zeroes) a rows x row_len table shard in the pool, fp32 or
  // (opt.table_dtype) bf16.
  // key_shift: workers send key = global_row << key_shift so the key-range
  // slicer shards rows evenly; this server's local row =
  // (key >> key_shift) - row_base, row_base derived from its key range.
  GpuSparseHandler(Postoffice* po, size_t rows, size_t row_len, bool accumulate,
                   int key_shift = 0, SparseOptConfig opt = SparseOptConfig());
  void operator()(const KVMeta& req, const KVPairs<float>& kvs, KVServer<float>* server);
  uintptr_t table_ptr() const { return reinterpret_cast<uintptr_t>(table_.data()); }
  // the optimizer state; 0 without one. Adagrad: rows floats row-wise, else
  // the table's shape. Lazy Adam: kern::SparseLazyAdam's records.
  uintptr_t state_ptr() const { return reinterpret_cast<uintptr_t>(state_.data()); }
  // learning rate of the gradient steps handled after the call
  void set_lr(float lr) { lr_.store(lr, std::memory_order_relaxed); }
  // Checkpoint: u64 rows, row_len, and a word of key_shift (low 32 bits) and
  // the table dtype (bit 32: bf16), then the table as it lies; with an
  // optimizer u64 state_floats and the state, as it lies, follow, and after
  // them on a bf16 table the u64 launch counter. Loading a file that ends
  // after the table resets the state to a fresh one, one that ends before
  // the counter sets it to 0; the file's dtype must be the handler's.
  void Save(const std::string& path);
  void Load(const std::string& path);

 private:
  hipStream_t Stream(int sender);
  // keys usable by a kernel: device keys pass through; host keys are
  // staged synchronously into a per-peer scratch row-id buffer
  const uint64_t* DeviceKeys(const SArray<Key>& keys, int sender, hipStream_t s);
  void GatherRespond(const KVMeta& req, const uint64_t* rows, size_t n, hipStream_t stream,
                     KVServer<float>* server);
  // answer a pull with the n rows that kernels on `stream` write into `out`
  void RespondRows(const KVMeta& req, const SArray<char>& out, size_t n, hipStream_t stream,
                   KVServer<float>* server);
  // the push of an optimizer handler; with req.pull it answers the pull too
  void OptimizerPush(const KVMeta& req, const KVPairs<float>& kvs, const uint64_t* rows,
                     hipStream_t stream, KVServer<float>* server);
  bool rowwise() const {
    return opt_.kind == SparseOpt::kRowwiseAdagrad || opt_.kind == SparseOpt::kRowwiseLazyAdam;
  }
  bool lazy_adam() const {
    return opt_.kind == SparseOpt::kLazyAdam || opt_.kind == SparseOpt::kRowwiseLazyAdam;
  }
  size_t state_floats() const {
    if (lazy_adam()) return kern::SparseLazyAdamStateFloats(rows_, row_len_, rowwise());
    return rowwise() ? rows_ : rows_ * row_len_;
  }
  // the state before any step, synchronously: init_acc (Adagrad), or
  // records of p1 = p2 = 1 and zeros (lazy Adam)
  void ResetState();
  // chain_: every kernel that touches the table waits for the one before
  // it (OrderAfter) and leaves its event for the next (Publish)
  void OrderAfter(hipStream_t s);
  void Publish(hipStream_t s);
  bool bf16() const { return opt_.table_dtype == SparseTableDtype::kBf16; }
  bool wire16() const { return opt_.wire_dtype == SparseTableDtype::kBf16; }
  // a message's n rows on the wire, in bytes
  size_t wire_bytes(size_t n) const {
    return n * row_len_ * (wire16() ? sizeof(uint16_t) : sizeof(float));
  }
  // the seed of the next launch that rounds; counts it
  uint64_t NextSeed() { return kern::SparseBf16LaunchSeed(opt_.seed, launches_.fetch_add(1)); }
  // The kernels' description of a call (kernels.h): our table, n message rows
  // on a stream, wire rows at p. rounds: the launch rounds on the store (an
  // add, a step), so on a bf16 table it takes the next seed.
  kern::SparseTable Table(bool rounds) {
    if (!bf16()) return {table_.data(), kern::SparseDtype::kF32};
    return {table_.data(), kern::SparseDtype::kBf16, opt_.rounding, rounds ? NextSeed() : 0};
  }
  kern::SparseRows Rows(const uint64_t* keys, size_t n, hipStream_t s) const {
    return {keys, n, row_len_, key_shift_, row_base_, rows_, s};
  }
  kern::SparseWire Wire(const void* p) const {
    return {const_cast<void*>(p), wire16() ? kern::SparseDtype::kBf16 : kern::SparseDtype::kF32};
  }

  Postoffice* po_;
  size_t rows_;
  size_t row_len_;
  bool accumulate_;
  bool atomic_ = false;  // >1 workers: concurrent scatters need atomics
  int key_shift_ = 0;
  uint64_t row_base_ = 0;
  SArray<char> table_;
  SparseOptConfig opt_;
  std::atomic<float> lr_{0.f};
  SArray<char> state_;
  std::atomic<uint64_t> launches_{0};  // bf16 table: launches that rounded so far
  // optimizer with > 1 workers: a step is a read-modify-write that atomics
  // cannot make safe, and the workers' messages run on different peer
  // streams, so one event orders every kernel on the table (the dense
  // handler's per-entry chain with the table as the one entry). A
  // message's step is then atomic with respect to other messages.
  bool chain_ = false;
  EventRef last_ev_;
  std::mutex mu_;
  std::unordered_map<int, SArray<char>> key_scratch_;  // per sender
  hipStream_t fallback_stream_ = nullptr;
};

}  // namespace xps
