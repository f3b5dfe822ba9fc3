// The MI355X data plane: same-host metadata over lock-free shm rings,
// payloads moved GPU-to-GPU over xGMI (hipIpc-mapped pools +
// hipMemcpyAsync / HIP kernels on per-peer side streams), completions
// via a hipEvent poller thread.
//
// Reference parity: replaces ps-lite's RDMA data path — rendezvous +
// one-sided RDMA_WRITE (src/rdma_van.h, rdma_transport.h) and the POSIX
// shm IPCTransport (rdma_transport.h:591-617) — per SURVEY.md §5.8:
//  * per-(key,peer) buffer rendezvous -> a single pool hipIpc handle
//    exchanged once at ADD_NODE (steady state ships {offset, len});
//  * unsignaled RDMA_WRITE + write-with-imm -> async copy/kernel on the
//    peer's stream + ring metadata sent after the completion event;
//  * PollCQ busy-spin thread -> the event-poller (completion) thread;
//  * IPCTransport shm segments -> the worker pool itself (zero copy).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <deque>
#include <memory>
#include <shared_mutex>
#include <thread>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "kernels.h"
#include "shm_ring.h"
#include "van.h"

namespace xps {

// zero-copy reception counter (by-ref blobs resolved straight into a
// mapped peer pool; see gpu_plane.cc)
extern std::atomic<uint64_t> g_zero_copy_recv;
// fused dual-write launches (kern::DenseAssign2) in this process: the
// dense handler's fused push+pull fast path plus the worker's one-sided
// GpuPlane::EntryPushPull
extern std::atomic<uint64_t> g_fused_assign;
// XPS_FUSED_ASSIGN (default 1): 0 restores the two-kernel push-then-pull
// everywhere (A/B runs within one build)
bool FusedAssignEnabled();
// dual-write LAUNCHES (direct or coalesced): equals g_fused_assign when
// every key has its own launch, smaller when queued keys shared launches
extern std::atomic<uint64_t> g_fused_launches;
// XPS_COALESCE (default 1): 0 gives every fused key its own launch and
// event again (A/B runs within one build)
bool CoalesceEnabled();

class Postoffice;

class GpuPlane : public DataPlane {
 public:
  GpuPlane(Postoffice* po, int device);
  ~GpuPlane() override;

  void FillSelf(Node* self) override;
  void ImportPeers() override;
  bool CanSend(const Message& msg, const Node& peer) override;
  int64_t Send(Message& msg, const Node& peer) override;
  void OnPeer(const Node& peer) override;
  void Stop() override;

  // ---- used by the GPU server handlers -------------------------------
  // Per-peer HIP stream LANES (XPS_STREAMS_PER_PEER, default 2):
  // lane 0 carries push/accumulate kernels, the pull lane carries pull-
  // response copies, so a key's response copy overlaps the next key's
  // push kernel (same xGMI link, different queues). Same-key cross-lane
  // ordering is the handlers' job via their last_ev event chains — the
  // dense handler enables chaining whenever lanes > 1. With 1 lane both
  // calls return the same stream (the round-1 behavior).
  hipStream_t StreamForPeer(int node_id);      // lane 0: push/compute
  hipStream_t PullStreamForPeer(int node_id);  // pull-response lane
  int lanes() const { return lanes_; }
  // do this peer's two lanes differ (cross-device)? Hands out no stream,
  // so unlike the two accessors above it leaves an open batch alone.
  bool LanesSplit(int node_id);

  // ---- dual-write launch coalescer (one open batch per lane-0 stream) --
  // Fused push+pull keys that arrive while the GPU is busy ride ONE
  // batched launch and ONE event. An open batch counts as already
  // enqueued on its stream: StreamForPeer / PullStreamForPeer (and every
  // internal lane-0 use) launch it before handing the stream out, so all
  // other stream work stays ordered behind it.
  // Handler side: append `seg` to the open batch of `peer_id`'s lane 0.
  // False = not batched (switch off, misaligned, ...): the open batch was
  // launched and the caller launches the segment itself. True = the
  // response the caller sends next ON THIS THREAD to that peer is
  // deferred on the batch's shared event; call CoalesceEnd right after.
  bool CoalesceAppend(int peer_id, const kern::Seg2& seg);
  // closes CoalesceAppend: if no deferred response picked the batch up
  // (it left on another path), launch the batch so the write still runs
  void CoalesceEnd(int peer_id);
  // per-peer traffic counters: (node id, tx bytes, rx bytes) — the
  // per-link utilization report of SURVEY §5.8 (each peer pair rides
  // its own xGMI link)
  std::vector<std::tuple<int, int64_t, int64_t>> PeerBytes();
  int device() const { return device_; }

  // One-sided pull (the RDMA_READ analog): copy `len` bytes from the
  // peer's advertised store entry straight into `dst` with OUR kernel
  // on the peer's lane-0 stream (ordered after our one-sided pushes of
  // the same key), then deliver the synthetic in-place response to
  // OURSELVES once the copy completes. Returns false when the peer's
  // pool is not mapped (caller sends a normal pull request).
  bool LocalPullRead(int peer_id, void* dst, uint64_t entry_off, size_t len, Message resp);
  // pooled events (shared with the server handlers)
  hipEvent_t GetEvent();
  void PutEvent(hipEvent_t ev);
  // resolve a peer-pool global offset to a locally mapped pointer
  // (handlers use this to write pull responses in place themselves)
  char* PeerDst(int peer_id, uint64_t global_off, uint64_t len) {
    return ResolvePeer(GetPeer(peer_id), global_off, len);
  }

 private:
  // completion of one coalesced launch, shared by every Pending of its
  // batch: ev stays null until the batch is launched, then holds the one
  // recorded event; it returns to the pool with the last reference
  struct CoEvent {
    explicit CoEvent(GpuPlane* pl) : plane(pl) {}
    ~CoEvent() {
      if (hipEvent_t e = ev.load(std::memory_order_acquire)) plane->PutEvent(e);
    }
    GpuPlane* plane;
    std::atomic<hipEvent_t> ev{nullptr};
    std::atomic<bool> done{false};  // set by the completion thread
    size_t bytes = 0;               // payload of the launch
  };
  struct Coalescer {
    std::mutex mu;
    kern::Seg2 segs[kern::kMaxBatch];
    int n = 0;
    std::atomic<int> n_open{0};  // == n, readable without mu
    size_t bytes = 0;
    std::shared_ptr<CoEvent> open;                 // event-to-be of the open batch
    std::deque<std::shared_ptr<CoEvent>> inflight;  // launched, not seen complete
    int64_t last_append_us = 0;                    // XPS_COALESCE_HOLD quiescence
  };

  struct Peer {
    Node node;
    Coalescer co;
    // set when this peer's Postoffice lives in OUR process (joint
    // mode): sends bypass serialize/ring/poll entirely (direct call)
    std::atomic<Postoffice*> local_po{nullptr};
    // producer handle on the peer's inbound ring. shared_ptr so a
    // RECOVERY (same id, new process, new shm_uid) can swap in a fresh
    // ring while in-flight pushes keep the old mapping alive (swapping
    // a by-value ring under a concurrent Push would munmap live memory)
    std::shared_ptr<ShmRing> ring;
    bool ring_tried = false;
    // fast-path flag: senders read this without taking mu
    std::atomic<bool> ring_ok{false};
    std::vector<void*> slab_bases;  // peer pool slabs mapped into our space
    bool pool_tried = false;
    // lane 0 = push, 1 = pull; created once, then read lock-free
    std::atomic<hipStream_t> streams[2] = {{nullptr}, {nullptr}};
    std::atomic<int64_t> tx_bytes{0};
    std::atomic<int64_t> rx_bytes{0};
    std::mutex mu;
  };

  // one message waiting for GPU work; the call sites of Defer name the
  // fields they set, Defer fills ev, peer_id and cev
  struct Pending {
    hipEvent_t ev = nullptr;  // null when cev is set
    int peer_id = 0;
    std::string payload;  // serialized ring form (empty for local_po)
    // TCP-resendable form of this message: if the ring push fails after
    // the event fires, the van sends this instead (never drop a response
    // — the requester is blocked in Wait). For in-place writes this is
    // the meta-only kOptInPlace message (the data already landed).
    // For same-process peers it is the message delivered directly.
    Message resend;
    Message keepalive;  // holds pool temporaries until the event fires
    int64_t bytes = 0;
    Postoffice* local_po = nullptr;  // same-process: deliver, don't ring-push
    std::shared_ptr<CoEvent> cev;    // coalesced launch this entry waits for
  };

  Peer* GetPeer(int id);
  // the peer's Postoffice when it lives in THIS process, else nullptr
  Postoffice* LocalPeer(Peer* p);
  // same-process send: no serialize, no ring — direct delivery (deferred
  // on the lane event when GPU kernels must complete first)
  int64_t SendLocal(Message& msg, Peer* p, Postoffice* lpo);
  void DeliverLocal(Postoffice* lpo, Message& msg, int64_t bytes);
  // hand a message to MY poll thread (I am the receiving side's plane):
  // keeps the sender's app thread free (pipelining) and runs the seq
  // gate on one thread. Falls back to inline delivery when the poll
  // thread is disabled.
  void EnqueueLocal(Message msg, int64_t bytes);
  bool EnsureRing(Peer* p);
  // the peer's current ring (nullptr when none could be opened)
  std::shared_ptr<ShmRing> RingOf(Peer* p);
  // import every slab of the peer's pool (idempotent)
  bool ImportPeerSlabs(Peer* p);
  // translate a peer-pool GLOBAL offset range to a mapped pointer
  // (nullptr if unmapped or the range is out of bounds / spans slabs)
  char* ResolvePeer(Peer* p, uint64_t global_off, uint64_t len);
  // serialize msg (meta + blobs, by-ref where flagged) into `out`;
  // by_ref[i] true => blob i encoded as pool offset
  bool Serialize(const Message& msg, const std::vector<char>& by_ref, std::string* out);
  void RingPollLoop();
  void CompletionLoop();
  // lane 0 launches the open batch first (see the coalescer above)
  hipStream_t StreamLane(int node_id, int lane);
  hipStream_t RawLane(Peer* p, int lane);  // no flush: the coalescing path only
  // coalescer internals; *Locked run under p->co.mu
  std::shared_ptr<CoEvent> CoAppend(Peer* p, const kern::Seg2& seg);
  void CoLaunchLocked(Peer* p);
  void CoPruneLocked(Peer* p);
  bool CoBusyLocked(Peer* p);  // prunes, then: is the GPU this stream's bottleneck?
  void CoFlush(Peer* p);
  // completion thread: an entry of an unlaunched batch reached the front
  // of its queue; true once the batch is launched
  bool CoFrontUnlaunched(Peer* p, const std::shared_ptr<CoEvent>& cev);
  void CoRetired(Peer* p);  // completion thread: a batch of p completed
  // this thread's pending CoalesceAppend ticket for peer_id, if any
  std::shared_ptr<CoEvent> TakeTicket(int peer_id);
  // One-sided fused push+pull (request carries kOptEntryPush with the
  // cached entry offset in meta.entry_addr and our own pull destination
  // in meta.addr): ONE dual-write kernel of ours stores vals to the
  // peer's mapped store entry and to the local destination, then the
  // meta-only kOptInPlace notification follows the completion event.
  // Returns false — nothing launched, nothing queued — when the entry or
  // the destination cannot be resolved or the peer has no ring.
  bool EntryPushPull(Message& msg, Peer* p, int64_t* bytes_out);
  // ---- the delivery rules of the send paths, each stated once --------
  // Queue `pd` until the work now on `stream` completed: record a pooled
  // event there — or wait on `cev`, the shared event of the coalesced
  // launch that carries this message's write (stream unused then).
  void Defer(Peer* p, hipStream_t stream, std::shared_ptr<CoEvent> cev, Pending pd);
  // Ring form of an in-place note, every blob inline. A note that
  // outgrows the ring sheds its blobs and travels as bare meta when
  // `may_drop_blobs`; otherwise not fitting is a bug.
  void SerializeNote(Message* note, bool may_drop_blobs, std::string* payload);
  // the lane a handler's response is ordered on: the pull lane when the
  // handler prepared its ordering there (kOptPullLane: the response copy
  // then overlaps the next push kernel on lane 0), else lane 0
  hipStream_t ResponseLane(const Message& msg, int peer_id);
  // copy host vals to offset `addr` of the requester's mapped host pool;
  // false when the pool cannot be mapped or the range leaves it
  bool CopyToHostDest(Peer* p, uint64_t addr, const SArray<char>& vals);
  // launch the copy of device vals into the HBM destination that pull
  // response `msg` answers, on its ResponseLane. nullptr: destination not
  // mapped — the peer's lanes were drained for the TCP fallback.
  hipStream_t WriteHbmDest(Peer* p, const Message& msg, const SArray<char>& vals);
  // Which plane's lane 0 carries OUR one-sided write to p's store, and
  // may it run at all (nullptr = no)? Cross-process: this plane, once
  // the peer's ring is up. Same process (*elpo set): the receiver's
  // plane, and only with XPS_LOCAL_ONE_SIDED=1.
  GpuPlane* OneSidedOwner(Peer* p, Postoffice** elpo);
  // that lane: taken only when the write is launched, because handing
  // out lane 0 launches its open batch
  hipStream_t OneSidedLane(GpuPlane* owner, Peer* p);
  // account a received message and hand it to the van; count_refs: count
  // its by-reference blobs as zero-copy receptions here
  void HandToVan(Van* van, Message& msg, int64_t bytes, bool count_refs);
  // a TCP fallback must not outrun kernels still running on this peer's
  // streams (the worker may reuse its buffers on the ack): drain them
  void DrainLanes(int peer_id);
  // a GPU handler's response waits for the handler's kernels
  bool DefersResponse(const Message& msg) const;

  Postoffice* po_;
  int device_;
  int lanes_ = 2;  // XPS_STREAMS_PER_PEER
  bool co_hold_ = false;             // XPS_COALESCE_HOLD (tests only)
  size_t co_byte_cap_ = 1ull << 30;  // XPS_COALESCE_CAP_MB
  uint64_t my_host_hash_;
  ShmRing in_ring_;
  bool started_ = false;
  bool inline_deliver_ = true;  // XPS_INLINE_HANDLER (default on)

  // read-mostly after bootstrap: shared lock on the hot send/recv paths
  std::shared_timed_mutex peers_mu_;
  std::unordered_map<int, std::unique_ptr<Peer>> peers_;

  std::thread poll_thread_;
  std::thread comp_thread_;
  std::atomic<bool> stop_{false};

  std::mutex pend_mu_;
  std::unordered_map<int, std::deque<Pending>> pending_;  // per peer, FIFO
  std::atomic<int> pending_count_{0};

  // same-process deliveries queued for MY poll thread
  std::mutex local_mu_;
  std::deque<std::pair<Message, int64_t>> local_q_;
  std::atomic<int> local_count_{0};
  bool poll_running_ = false;  // poll thread exists (set in FillSelf)

  std::mutex ev_mu_;
  std::vector<hipEvent_t> event_pool_;
};

// Returns the plane for this van, or nullptr when no GPU is attached.
std::shared_ptr<DataPlane> CreateGpuPlane(Postoffice* po, int device);

}  // namespace xps
