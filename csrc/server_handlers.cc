#include "server_handlers.h"

#include "gpu_plane.h"
#include "hip_check.h"
#include "hip_pool.h"
#include "kernels.h"
#include "mxfp8.h"

namespace xps {

std::atomic<uint64_t> g_mx_launches{0};

static GpuPlane* ThePlane(Postoffice* po) {
  return dynamic_cast<GpuPlane*>(po->van() ? po->van()->plane() : nullptr);
}

// The peer's lane 0 (push kernels) or its pull-response lane: copies there
// overlap the next push kernel on lane 0; same-key ordering rides the
// handler's event chain. Without a plane one fallback stream serves both.
static hipStream_t LaneStream(Postoffice* po, int sender, bool pull, hipStream_t* fallback) {
  if (auto* plane = ThePlane(po)) {
    return pull ? plane->PullStreamForPeer(sender) : plane->StreamForPeer(sender);
  }
  if (!*fallback) {
    XPS_HIP_CHECK(hipStreamCreateWithFlags(fallback, hipStreamNonBlocking));
  }
  return *fallback;
}

static hipEvent_t EventAlloc(Postoffice* po) {
  if (auto* plane = ThePlane(po)) return plane->GetEvent();
  hipEvent_t ev;
  XPS_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  return ev;
}

static void EventFree(Postoffice* po, hipEvent_t ev) {
  if (auto* plane = ThePlane(po)) {
    plane->PutEvent(ev);
  } else {
    (void)hipEventDestroy(ev);
  }
}

// ------------------------------------------------------------------ dense

// Did the requester advertise an in-place HBM destination (kOptHostAddr
// names an offset in the host pool instead)? Without one the van stages the
// response's device vals through host memory; its device-to-host copy is
// stream-unaware, so the handler drains its stream first.
static bool HbmDest(int option) {
  return (option & kOptPullAddr) && !(option & kOptHostAddr);
}

// byte length of key i of n: lens omitted = equal split of vals
static inline size_t LenOf(const KVPairs<float>& kvs, size_t i, size_t n) {
  return kvs.lens.empty() ? kvs.vals.nbytes() / n
                          : static_cast<size_t>(kvs.lens[i]) * sizeof(float);
}

// descs hold dst and nbytes: segment i reads vals where segment i-1 ended
static void SliceInto(std::vector<kern::CopyDesc>* descs, const void* vals) {
  size_t off = 0;
  for (auto& d : *descs) {
    d.src = static_cast<const char*>(vals) + off;
    off += d.nbytes;
  }
}

// one batched kernel for the list, or one launch per segment when a pointer
// or length is off the 16 B grid
static void CopySegments(const std::vector<kern::CopyDesc>& descs, hipStream_t s) {
  if (kern::BatchAligned(descs.data(), descs.size())) {
    kern::BatchedAssign(descs.data(), static_cast<int>(descs.size()), s);
  } else {
    for (auto& d : descs) kern::DenseAssign(d.dst, d.src, d.nbytes, s);
  }
}

// descs hold src and nbytes: pack them back to back into a fresh pool buffer
// (the plane keeps it alive until the response is sent)
static SArray<float> PackStaged(std::vector<kern::CopyDesc>* descs, hipStream_t s) {
  size_t total = 0;
  for (auto& d : *descs) total += d.nbytes;
  SArray<char> tmp = HbmPool::Get()->AllocArray(total);
  size_t off = 0;
  for (auto& d : *descs) {
    d.dst = tmp.data() + off;
    off += d.nbytes;
  }
  CopySegments(*descs, s);
  return SArray<float>::View(tmp);
}

// Answer a pull with vals that the plane writes in place on `stream`, or
// that the van stages through the host (TCP fallback)
static void RespondStaged(KVMeta r, const KVPairs<float>& res, hipStream_t stream,
                          KVServer<float>* server) {
  if (!HbmDest(r.option)) XPS_HIP_CHECK(hipStreamSynchronize(stream));
  r.option |= kOptPullLane;  // ordering prepared on the pull lane
  server->Response(r, res);  // plane enqueues the in-place read on `stream`
}

static EventRef MakeEventRef(Postoffice* po, hipStream_t s) {
  hipEvent_t ev = EventAlloc(po);
  XPS_HIP_CHECK(hipEventRecord(ev, s));
  return EventRef(ev, [po](hipEvent_t e) { EventFree(po, e); });
}

GpuDenseHandler::GpuDenseHandler(Postoffice* po, DenseMode mode, DenseDtype dtype)
    : po_(po), mode_(mode), dtype_(dtype) {
  XPS_CHECK(HbmPool::Get()->initialized()) << "GpuDenseHandler needs the HBM pool";
  XPS_CHECK(dtype_ != DenseDtype::kMxfp8 || mode_ == DenseMode::kReduce)
      << "mxfp8 payloads exist in reduce mode only";
  num_workers_ = std::max(1, po_->num_workers());
  // >1 workers: same-key kernels land on different peers' streams
  chain_ = num_workers_ > 1;
}

void GpuDenseHandler::SumKernel(void* dst, const void* src, size_t nbytes, hipStream_t s) {
  XPS_CHECK(dtype_ != DenseDtype::kMxfp8) << "mxfp8 has no in-place sum";
  if (dtype_ == DenseDtype::kBf16) {
    kern::DenseSumBf16(static_cast<uint16_t*>(dst), static_cast<const uint16_t*>(src),
                       nbytes / 2, s);
  } else {
    kern::DenseSumF32(static_cast<float*>(dst), static_cast<const float*>(src), nbytes / 4, s);
  }
}

void GpuDenseHandler::BatchedSum(const kern::CopyDesc* descs, int n, hipStream_t s) {
  XPS_CHECK(dtype_ != DenseDtype::kMxfp8) << "mxfp8 has no in-place sum";
  if (dtype_ == DenseDtype::kBf16) {
    kern::BatchedSumBf16(descs, n, s);
  } else {
    kern::BatchedSumF32(descs, n, s);
  }
}

void GpuDenseHandler::SumSegments(const std::vector<kern::CopyDesc>& descs, hipStream_t s) {
  if (kern::BatchAligned(descs.data(), descs.size())) {
    BatchedSum(descs.data(), static_cast<int>(descs.size()), s);
  } else {
    for (auto& d : descs) SumKernel(d.dst, d.src, d.nbytes, s);
  }
}

bool GpuDenseHandler::NeedChain(int sender) {
  if (chain_) return true;
  // lane split for this peer (cross-device): push kernels on lane 0 and
  // pull copies on the pull lane touch the same entries — chain them
  auto* plane = ThePlane(po_);
  return plane && plane->LanesSplit(sender);
}

GpuDenseHandler::~GpuDenseHandler() = default;

void GpuDenseHandler::OrderAfter(Entry* e, hipStream_t s) {
  if (e->last_ev) XPS_HIP_CHECK(hipStreamWaitEvent(s, e->last_ev.get(), 0));
}

GpuDenseHandler::Entry* GpuDenseHandler::EntryLocked(Key key, size_t len) {
  Entry* e = &store_[key];
  if (e->buf.size() >= len) return e;
  // retire (never free) a smaller buffer: workers may hold its offset in
  // their one-sided entry caches — a stale write must land in
  // dead-but-owned memory, not a reused pool region
  if (!e->buf.empty()) e->retired.push_back(e->buf);
  e->buf = HbmPool::Get()->AllocArray(len);
  // zero before publishing: another peer's stream may accumulate into
  // this entry concurrently with our first push
  XPS_HIP_CHECK(hipMemset(e->buf.data(), 0, len));
  return e;
}

GpuDenseHandler::Entry* GpuDenseHandler::EntryFor(Key key, size_t len) {
  std::lock_guard<std::mutex> lk(mu_);
  return EntryLocked(key, len);
}

void GpuDenseHandler::GrowReduce(Entry* e, size_t len) {
  // no retire and no zeroing, unlike EntryLocked: a round's first push
  // overwrites, and a hipMemset is a blocking call on the hot path
  if (e->buf.size() < len) e->buf = HbmPool::Get()->AllocArray(len);
}

hipStream_t GpuDenseHandler::Stream(int sender) {
  return LaneStream(po_, sender, /*pull=*/false, &fallback_stream_);
}

hipStream_t GpuDenseHandler::PullStream(int sender) {
  return LaneStream(po_, sender, /*pull=*/true, &fallback_stream_);
}

void GpuDenseHandler::operator()(const KVMeta& req, const KVPairs<float>& kvs,
                                 KVServer<float>* server) {
  if (req.push && req.pull) {
    // fused ZPushPull: apply the push silently, then answer with the
    // post-push values (same stream -> ordered). Reduce mode holds
    // pulls for round accounting and cannot fuse them into one message.
    XPS_CHECK(mode_ != DenseMode::kReduce)
        << "ZPushPull is not supported in reduce mode (pulls are held per round)";
    if (req.option & kOptInPlace) {
      // one-sided fused round: the worker's dual-write kernel already
      // stored vals into our entry AND its own destination (the
      // notification is ordered after that kernel's completion event);
      // nothing to launch — answer meta-only, in place
      server->Response(req);
      return;
    }
    if (TryFusedAssign(req, kvs, server)) return;
    HandlePush(req, kvs, server, /*respond=*/false);
    HandlePull(req, kvs, server);
    return;
  }
  if (req.push) {
    HandlePush(req, kvs, server);
  } else if (req.pull) {
    HandlePull(req, kvs, server);
  } else {
    server->Response(req);
  }
}

// Fused push+pull of ONE key in ONE launch: store[key] = dst = src with
// the dual-write kernel, instead of the push kernel plus the pull kernel
// that re-read the 'just written' entry. Returns false (nothing done) when
// any precondition fails; the caller then runs the two-step path.
bool GpuDenseHandler::TryFusedAssign(const KVMeta& req, const KVPairs<float>& kvs,
                                     KVServer<float>* server) {
  if (!FusedAssignEnabled()) return false;
  if (mode_ != DenseMode::kAssign || req.cmd == kCmdSum) return false;
  if (kvs.keys.size() != 1 || !kvs.vals.on_device()) return false;
  if (!HbmDest(req.option)) return false;
  size_t len = LenOf(kvs, 0, 1);
  if (len == 0 || len != kvs.vals.nbytes() || static_cast<int64_t>(len) != req.val_len) {
    return false;
  }
  auto* plane = ThePlane(po_);
  if (!plane) return false;
  char* dst = plane->PeerDst(req.sender, req.addr, len);
  if (!dst) return false;
  XPS_STAGE(dense_fused_assign);
  XPS_HIP_CHECK(hipSetDevice(HbmPool::Get()->device()));
  Entry* e = EntryFor(kvs.keys[0], len);
  // a LARGER entry keeps its tail: the pull would return more than was
  // pushed — that is the two-step path's business
  if (e->buf.size() != len) return false;
  const char* src = reinterpret_cast<const char*>(kvs.vals.data());
  if (!kern::Disjoint3(e->buf.data(), dst, src, len)) return false;
  // Queued behind a busy GPU the key joins the open batch of the sender's
  // lane and shares its launch and event (GpuPlane's coalescer). Senders
  // that need the last_ev chain keep their own launch: the chain wants an
  // event per key.
  bool chain = NeedChain(req.sender);
  bool coalesced = !chain && !e->last_ev &&
                   plane->CoalesceAppend(req.sender, kern::Seg2{e->buf.data(), dst, src, len});
  if (!coalesced) {
    hipStream_t stream = Stream(req.sender);
    OrderAfter(e, stream);
    kern::DenseAssign2(e->buf.data(), dst, src, len, stream);
    g_fused_launches.fetch_add(1, std::memory_order_relaxed);
    if (chain) e->last_ev = MakeEventRef(po_, stream);
  }
  g_fused_assign.fetch_add(1, std::memory_order_relaxed);
  g_zero_copy_recv.fetch_add(1, std::memory_order_relaxed);
  // meta-only in-place response; the work ran on the PUSH lane, so no
  // kOptPullLane — the plane defers delivery on that lane's event. The
  // entry advert rides along so the worker can go one-sided next time (in
  // entry_addr: addr and val_len still describe the pull).
  KVMeta r = req;
  r.option |= kOptInPlace;
  r.option &= ~(kOptPullLane | kOptEntryPush);
  r.val_len = static_cast<int64_t>(len);
  uint64_t eoff = 0;
  if (HbmPool::Get()->OffsetOf(e->buf.data(), &eoff)) {
    r.entry_addr = eoff;
    r.option |= kOptEntryAddr;
  }
  server->Response(r);
  if (coalesced) plane->CoalesceEnd(req.sender);
  return true;
}

GpuDenseHandler::Group* GpuDenseHandler::GroupFor(const SArray<Key>& keys) {
  // FNV-1a over the key bytes identifies the key-set
  uint64_t h = 1469598103934665603ull;
  const unsigned char* p = reinterpret_cast<const unsigned char*>(keys.data());
  for (size_t i = 0; i < keys.nbytes(); ++i) {
    h ^= p[i];
    h *= 1099511628211ull;
  }
  Group* g;
  {
    std::lock_guard<std::mutex> lk(mu_);
    g = &groups_[h];
  }
  if (g->keys.empty()) {
    g->keys.assign(keys.begin(), keys.end());
    g->ents.reserve(keys.size());
    std::lock_guard<std::mutex> lk(mu_);
    for (Key k : g->keys) g->ents.push_back(&store_[k]);
  } else {
    XPS_CHECK(g->keys.size() == keys.size() &&
              std::equal(g->keys.begin(), g->keys.end(), keys.begin()))
        << "reduce mode needs a consistent key->message grouping across workers "
           "(key-set hash collision or inconsistent bucketing)";
  }
  return g;
}

void GpuDenseHandler::HandleReducePush(const KVMeta& req, const KVPairs<float>& kvs,
                                       KVServer<float>* server) {
  XPS_STAGE(reduce_push);
  size_t n = kvs.keys.size();
  Group* g = GroupFor(kvs.keys);
  if (g->pushes >= num_workers_) {
    // a fast worker started the next round before this round's pulls
    // drained: defer (the KVPairs copy keeps the remote buffer alive)
    g->waiting_pushes.emplace_back(req, kvs);
    return;
  }
  XPS_CHECK(kvs.vals.on_device()) << "reduce mode needs device vals (pool buffers)";
  if (g->lens.size() != n) {
    g->lens.resize(n);
    for (size_t i = 0; i < n; ++i) g->lens[i] = LenOf(kvs, i, n);
  }
  hipStream_t stream = Stream(req.sender);
  XPS_HIP_CHECK(hipSetDevice(HbmPool::Get()->device()));
  if (g->last_ev) XPS_HIP_CHECK(hipStreamWaitEvent(stream, g->last_ev.get(), 0));
  bool first = g->pushes == 0;
  if (first) {
    // the previous round's pull copies must finish before we overwrite
    for (auto& ev : g->pull_guard) {
      XPS_HIP_CHECK(hipStreamWaitEvent(stream, ev.get(), 0));
    }
    g->pull_guard.clear();
  }
  if (dtype_ == DenseDtype::kMxfp8) {
    ReducePushMx(g, kvs, stream);
    FinishReducePush(req, g, server, stream);
    return;
  }
  // one batched kernel chain for the whole key-set (3 launches for 169
  // rn50 buckets at kMaxBatch=64), one event per push
  std::vector<kern::CopyDesc> descs;
  descs.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    GrowReduce(g->ents[i], g->lens[i]);
    descs.push_back({g->ents[i]->buf.data(), nullptr, g->lens[i]});
  }
  SliceInto(&descs, kvs.vals.data());
  if (first) {
    CopySegments(descs, stream);
  } else {
    SumSegments(descs, stream);
  }
  FinishReducePush(req, g, server, stream);
}

// MXFP8 round: the first push decodes into the fp32 accumulator, middle
// pushes add to it, and the push that completes the round writes
// Q(acc + D(push)) into the entries' packed buffers — each gradient is
// rounded once at its worker and once here, however many workers add up.
// With one worker the round is that last step alone.
void GpuDenseHandler::ReducePushMx(Group* g, const KVPairs<float>& kvs, hipStream_t stream) {
  size_t n = g->keys.size();
  bool first = g->pushes == 0;
  bool last = g->pushes + 1 >= num_workers_;
  const char* vals = reinterpret_cast<const char*>(kvs.vals.data());
  XPS_CHECK((reinterpret_cast<uintptr_t>(vals) & 15u) == 0)
      << "mxfp8 push: vals must be 16 B-aligned";
  std::vector<kern::MxSeg> segs;
  segs.reserve(n);
  size_t off = 0;
  for (size_t i = 0; i < n; ++i) {
    size_t len = g->lens[i];
    XPS_CHECK(len % mx::kSuperBytes == 0)
        << "mxfp8 push: key " << g->keys[i] << " has " << len
        << " payload bytes, not a multiple of the 528-byte superblock";
    Entry* e = g->ents[i];
    GrowReduce(e, len);
    XPS_CHECK((reinterpret_cast<uintptr_t>(e->buf.data()) & 15u) == 0)
        << "mxfp8 push: the entry of key " << g->keys[i] << " is not 16 B-aligned";
    size_t acc_len = len / mx::kSuperBytes * mx::kSuperF32Bytes;
    if (!(first && last) && e->acc.size() < acc_len) e->acc = HbmPool::Get()->AllocArray(acc_len);
    float* acc = first && last ? nullptr : reinterpret_cast<float*>(e->acc.data());
    segs.push_back({acc, vals + off, e->buf.data(), len});
    off += len;
  }
  XPS_CHECK_LE(off, kvs.vals.nbytes()) << "mxfp8 push: lens exceed the payload";
  int launches = last ? kern::BatchedMxFinish(segs.data(), static_cast<int>(n), stream)
                      : kern::BatchedMxAccumulate(segs.data(), static_cast<int>(n), first, stream);
  g_mx_launches.fetch_add(static_cast<uint64_t>(launches), std::memory_order_relaxed);
}

void GpuDenseHandler::FinishReducePush(const KVMeta& req, Group* g, KVServer<float>* server,
                                       hipStream_t stream) {
  g->pushes++;
  EventRef ev = MakeEventRef(po_, stream);
  g->round_events.push_back(ev);
  g->last_ev = ev;
  server->Response(req);
  if (g->pushes >= num_workers_) {
    std::vector<KVMeta> waiting;
    waiting.swap(g->waiting_pulls);
    for (auto& w : waiting) RespondPull(w, g, server);
  }
}

void GpuDenseHandler::HandlePush(const KVMeta& req, const KVPairs<float>& kvs,
                                 KVServer<float>* server, bool respond) {
  XPS_STAGE(dense_push);
  size_t n = kvs.keys.size();
  XPS_CHECK_GT(n, 0u);
  if (mode_ == DenseMode::kReduce) {
    HandleReducePush(req, kvs, server);
    return;
  }
  if (req.option & kOptInPlace) {
    // one-sided push: the worker's kernel already wrote our store entry
    // (the notification is ordered after the write's completion event);
    // nothing to launch — ack immediately
    if (respond) server->Response(req);
    return;
  }
  hipStream_t stream = Stream(req.sender);
  XPS_HIP_CHECK(hipSetDevice(HbmPool::Get()->device()));
  bool chain = NeedChain(req.sender);
  bool sum_all = mode_ == DenseMode::kAssign ? req.cmd == kCmdSum : req.cmd != kCmdAssign;
  // multi-key device push: one batched kernel launch for all segments. A
  // list off the 16 B grid falls through to the per-key loop, not to
  // per-segment launches: when chaining, that loop orders and publishes an
  // event per key.
  if (kvs.vals.on_device() && n > 1) {
    std::vector<kern::CopyDesc> descs;
    std::vector<Entry*> ents;
    descs.reserve(n);
    ents.reserve(n);
    for (size_t i = 0; i < n; ++i) {
      size_t len = LenOf(kvs, i, n);
      ents.push_back(EntryFor(kvs.keys[i], len));
      descs.push_back({ents[i]->buf.data(), nullptr, len});
    }
    SliceInto(&descs, kvs.vals.data());
    if (kern::BatchAligned(descs.data(), n)) {
      for (Entry* e : ents) OrderAfter(e, stream);
      if (sum_all) {
        BatchedSum(descs.data(), static_cast<int>(n), stream);
      } else {
        kern::BatchedAssign(descs.data(), static_cast<int>(n), stream);
      }
      if (chain) {
        EventRef ev = MakeEventRef(po_, stream);  // one event covers the batch
        for (Entry* e : ents) e->last_ev = ev;
      }
      if (!ThePlane(po_)) XPS_HIP_CHECK(hipStreamSynchronize(stream));
      if (respond) server->Response(req);
      return;
    }
  }
  size_t off = 0;  // bytes into vals
  bool synced = false;
  Entry* last_e = nullptr;
  for (size_t i = 0; i < n; ++i) {
    size_t len = LenOf(kvs, i, n);
    Entry* e = last_e = EntryFor(kvs.keys[i], len);
    const char* src = reinterpret_cast<const char*>(kvs.vals.data()) + off;
    if (kvs.vals.on_device()) {
      OrderAfter(e, stream);
      {
        XPS_STAGE(push_kernel_launch);
        if (sum_all) {
          SumKernel(e->buf.data(), src, len, stream);
        } else {
          kern::DenseAssign(e->buf.data(), src, len, stream);
        }
      }
      if (chain) {
        XPS_STAGE(push_chain_event);
        e->last_ev = MakeEventRef(po_, stream);
      }
    } else {
      // host vals land via synchronous copies below: drain the entry's
      // outstanding cross-stream kernel first
      if (chain && e->last_ev) {
        XPS_HIP_CHECK(hipEventSynchronize(e->last_ev.get()));
        e->last_ev.reset();
      }
      // host vals (TCP-staged path): correctness-first synchronous route
      if (sum_all) {
        SArray<char> scratch = HbmPool::Get()->AllocArray(len);
        XPS_HIP_CHECK(hipMemcpy(scratch.data(), src, len, hipMemcpyHostToDevice));
        SumKernel(e->buf.data(), scratch.data(), len, stream);
        XPS_HIP_CHECK(hipStreamSynchronize(stream));
        synced = true;
      } else {
        XPS_HIP_CHECK(hipMemcpy(e->buf.data(), src, len, hipMemcpyHostToDevice));
      }
    }
    off += len;
  }
  auto* plane = ThePlane(po_);
  if (!plane && !synced) XPS_HIP_CHECK(hipStreamSynchronize(stream));
  if (!respond) return;
  // assign mode, single key: advertise the store entry's pool offset so
  // this worker's next pushes of the key go one-sided (kOptEntryPush). This
  // advert names the entry in addr and val_len; the fused path's rides in
  // entry_addr beside the pull's own addr.
  if (mode_ == DenseMode::kAssign && n == 1 && last_e && plane) {
    uint64_t eoff = 0;
    if (HbmPool::Get()->OffsetOf(last_e->buf.data(), &eoff)) {
      KVMeta r = req;
      r.addr = eoff;
      r.val_len = static_cast<int64_t>(last_e->buf.size());
      r.option |= kOptEntryAddr;
      server->Response(r);
      return;
    }
  }
  server->Response(req);
}

// Pull written straight into the requester's advertised HBM pool range: one
// batched copy of every segment (descs hold src and nbytes) and a meta-only
// response that the plane defers on `stream`. False, with nothing launched or
// sent, when there is no such destination, a segment does not resolve in the
// peer's pool, or the list is off the 16 B grid. That the destination holds
// every segment is the caller's to know.
bool GpuDenseHandler::TryPullInPlace(const KVMeta& req, const KVPairs<float>& res,
                                     std::vector<kern::CopyDesc>* descs, hipStream_t stream,
                                     KVServer<float>* server) {
  auto* plane = ThePlane(po_);
  if (!plane || !HbmDest(req.option)) return false;
  uint64_t off = 0;
  for (auto& d : *descs) {
    d.dst = plane->PeerDst(req.sender, req.addr + off, d.nbytes);
    if (!d.dst) return false;
    off += d.nbytes;
  }
  if (!kern::BatchAligned(descs->data(), descs->size())) return false;
  kern::BatchedAssign(descs->data(), static_cast<int>(descs->size()), stream);
  KVMeta r = req;
  r.option |= kOptInPlace | kOptPullLane;
  r.val_len = static_cast<int64_t>(off);
  server->Response(r, res);  // keys and lens only
  return true;
}

void GpuDenseHandler::RespondPull(const KVMeta& req, Group* g, KVServer<float>* server) {
  XPS_STAGE(reduce_respond_pull);
  hipStream_t stream = PullStream(req.sender);
  for (auto& ev : g->round_events) {
    XPS_HIP_CHECK(hipStreamWaitEvent(stream, ev.get(), 0));
  }
  size_t n = g->keys.size();
  KVPairs<float> res;
  res.keys = SArray<Key>(g->keys);
  SArray<int> lens(n);
  std::vector<kern::CopyDesc> descs;
  descs.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    lens[i] = static_cast<int>(g->lens[i] / sizeof(float));
    descs.push_back({nullptr, g->ents[i]->buf.data(), g->lens[i]});
  }
  res.lens = lens;
  // req.val_len does not bound the in-place write here; in HandlePull it does
  if (!TryPullInPlace(req, res, &descs, stream, server)) {
    // staging path (TCP fallback / no advertised destination / off the 16 B grid)
    res.vals = n == 1 ? SArray<float>::View(g->ents[0]->buf) : PackStaged(&descs, stream);
    RespondStaged(req, res, stream, server);
  }
  EventRef pe = MakeEventRef(po_, stream);
  g->pull_guard.push_back(pe);
  g->last_ev = pe;
  g->pulled_senders.insert(req.sender);
  g->pulls++;
  if (g->pulls >= num_workers_) {
    // round over: reset, then replay deferred next-round pushes + pulls
    g->pushes = 0;
    g->pulls = 0;
    g->pulled_senders.clear();
    g->round_events.clear();  // refs drop back to the event pool
    std::vector<std::pair<KVMeta, KVPairs<float>>> dpush;
    dpush.swap(g->waiting_pushes);
    for (auto& d : dpush) HandleReducePush(d.first, d.second, server);
    std::vector<KVMeta> dpull;
    dpull.swap(g->waiting_next_pulls);
    for (auto& d : dpull) {
      if (g->pushes >= num_workers_) {
        RespondPull(d, g, server);
      } else {
        g->waiting_pulls.push_back(d);
      }
    }
  }
}

void GpuDenseHandler::HandlePull(const KVMeta& req, const KVPairs<float>& kvs,
                                 KVServer<float>* server) {
  XPS_STAGE(dense_pull);
  size_t n = kvs.keys.size();
  XPS_CHECK_GT(n, 0u);
  XPS_HIP_CHECK(hipSetDevice(HbmPool::Get()->device()));
  if (mode_ == DenseMode::kReduce) {
    // a pull may legitimately precede the round's pushes (it just
    // waits); GroupFor creates the round group on demand. NOTE: no lock
    // is held across RespondPull — its round-reset path replays deferred
    // pushes through HandleReducePush (which locks mu_ for store_
    // access); Group state itself is serialized by the handler lane.
    Group* g = GroupFor(kvs.keys);
    if (g->pulled_senders.count(req.sender)) {
      // this sender already pulled the current round: a NEXT-round pull
      g->waiting_next_pulls.push_back(req);
      return;
    }
    if (g->pushes < num_workers_) {
      g->waiting_pulls.push_back(req);  // released by the round's last push
      return;
    }
    RespondPull(req, g, server);
    return;
  }
  hipStream_t stream = PullStream(req.sender);
  bool chain = NeedChain(req.sender);
  KVPairs<float> res;
  res.keys = kvs.keys;
  SArray<int> lens(n);
  std::vector<Entry*> touched;
  SArray<char> entry;                  // n == 1: served as a zero-copy store view
  std::vector<kern::CopyDesc> descs;  // n > 1: whole entries, in key order
  if (n > 1) descs.reserve(n);
  size_t total = 0;
  {
    std::lock_guard<std::mutex> lk(mu_);
    for (size_t i = 0; i < n; ++i) {
      auto it = store_.find(kvs.keys[i]);
      XPS_CHECK(it != store_.end()) << "pull of unknown key " << kvs.keys[i];
      const SArray<char>& buf = it->second.buf;
      touched.push_back(&it->second);
      lens[i] = static_cast<int>(buf.size() / sizeof(float));
      total += buf.size();
      if (n == 1) {
        entry = buf;
      } else {
        descs.push_back({nullptr, buf.data(), buf.size()});
      }
    }
  }
  res.lens = lens;
  // the copies below (ours, the plane's in-place write, or the sync) read
  // the entries on `stream`: order it behind their last writers
  {
    XPS_STAGE(pull_order_after);
    for (Entry* e : touched) OrderAfter(e, stream);
  }
  // the advertised destination can be SMALLER than the store entries (an
  // entry grew since the worker sized its buffer): an in-place write would
  // overrun the requester's pool region
  bool fits = !(req.val_len > 0 && static_cast<int64_t>(total) > req.val_len);
  // several keys go straight into the requester's mapped pool when they fit
  // (no staging buffer); one key is the plane's in-place write of the view
  if (!(n > 1 && fits && TryPullInPlace(req, res, &descs, stream, server))) {
    res.vals = n == 1 ? SArray<float>::View(entry) : PackStaged(&descs, stream);
    KVMeta r = req;
    // too small a destination: force the staging path, whose worker-side
    // merge checks the overflow loudly
    if (!fits) r.option &= ~kOptPullAddr;
    RespondStaged(r, res, stream, server);
  }
  // after the response in either branch
  if (chain) {
    EventRef ev = MakeEventRef(po_, stream);  // pushes must wait these reads
    for (Entry* e : touched) e->last_ev = ev;
  }
}

void GpuDenseHandler::RegisterEntry(Key key, void* ptr, size_t nbytes, int device) {
  XPS_CHECK(ptr && nbytes) << "RegisterEntry needs a real buffer";
  std::lock_guard<std::mutex> lk(mu_);
  Entry& e = store_[key];
  if (!e.buf.empty()) e.retired.push_back(e.buf);  // keep old offsets owned
  // non-owning view: the app keeps the buffer alive
  e.buf = SArray<char>(static_cast<char*>(ptr), nbytes, device);
}

void GpuDenseHandler::Save(const std::string& path) {
  FILE* f = fopen(path.c_str(), "wb");
  XPS_CHECK(f) << "cannot open checkpoint " << path;
  std::lock_guard<std::mutex> lk(mu_);
  uint64_t n = store_.size();
  fwrite(&n, 8, 1, f);
  std::vector<char> host;
  for (auto& kv : store_) {
    uint64_t key = kv.first, len = kv.second.buf.size();
    fwrite(&key, 8, 1, f);
    fwrite(&len, 8, 1, f);
    host.resize(len);
    XPS_HIP_CHECK(hipMemcpy(host.data(), kv.second.buf.data(), len, hipMemcpyDeviceToHost));
    fwrite(host.data(), 1, len, f);
  }
  fclose(f);
}

void GpuDenseHandler::Load(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  XPS_CHECK(f) << "cannot open checkpoint " << path;
  std::lock_guard<std::mutex> lk(mu_);
  uint64_t n = 0;
  XPS_CHECK_EQ(fread(&n, 8, 1, f), 1u);
  std::vector<char> host;
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t key, len;
    XPS_CHECK_EQ(fread(&key, 8, 1, f), 1u);
    XPS_CHECK_EQ(fread(&len, 8, 1, f), 1u);
    host.resize(len);
    XPS_CHECK_EQ(fread(host.data(), 1, len, f), len);
    Entry* e = EntryLocked(key, len);
    XPS_HIP_CHECK(hipMemcpy(e->buf.data(), host.data(), len, hipMemcpyHostToDevice));
  }
  fclose(f);
}

// ----------------------------------------------------------------- sparse

GpuSparseHandler::GpuSparseHandler(Postoffice* po, size_t rows, size_t row_len, bool accumulate,
                                   int key_shift)
    : po_(po), rows_(rows), row_len_(row_len), accumulate_(accumulate), key_shift_(key_shift) {
  auto* pool = HbmPool::Get();
  XPS_CHECK(pool->initialized()) << "GpuSparseHandler needs the HBM pool";
  // concurrent workers scatter on different peer streams: accumulate
  // must be element-atomic or overlapping rows lose updates
  atomic_ = po_->num_workers() > 1;
  if (key_shift_ > 0) {
    int rank = po_->my_rank();
    // the first row whose key (row << key_shift) lies in our range. Range
    // begins are multiples of (2^64 - 1) / num_servers, which fall one
    // short of the row boundary for a power-of-two split: round up, or
    // every local row sits one too high and the shard's last row is lost.
    uint64_t begin = po_->GetServerKeyRanges()[rank].begin;
    uint64_t low = (1ull << key_shift_) - 1;
    row_base_ = (begin >> key_shift_) + ((begin & low) ? 1 : 0);
  }
  XPS_HIP_CHECK(hipSetDevice(pool->device()));
  table_ = pool->AllocArray(rows * row_len * sizeof(float));
  XPS_HIP_CHECK(hipMemset(table_.data(), 0, table_.size()));
}

hipStream_t GpuSparseHandler::Stream(int sender) {
  return LaneStream(po_, sender, /*pull=*/false, &fallback_stream_);
}

const uint64_t* GpuSparseHandler::DeviceKeys(const SArray<Key>& keys, int sender,
                                             hipStream_t s) {
  if (keys.on_device()) return keys.data();
  // host keys: stage synchronously into the per-sender scratch (ordered
  // before any kernel we launch afterwards on `s`)
  size_t bytes = keys.nbytes();
  SArray<char> scratch;
  {
    std::lock_guard<std::mutex> lk(mu_);
    auto& sc = key_scratch_[sender];
    if (sc.size() < bytes) sc = HbmPool::Get()->AllocArray(std::max<size_t>(bytes, 1 << 16));
    scratch = sc;
  }
  XPS_HIP_CHECK(hipStreamSynchronize(s));  // prior kernels still reading the scratch
  XPS_HIP_CHECK(hipMemcpy(scratch.data(), keys.data(), bytes, hipMemcpyHostToDevice));
  return reinterpret_cast<const uint64_t*>(scratch.data());
}

// gather the n rows on `stream` and answer the pull with them
void GpuSparseHandler::GatherRespond(const KVMeta& req, const uint64_t* rows, size_t n,
                                     hipStream_t stream, KVServer<float>* server) {
  SArray<char> out = HbmPool::Get()->AllocArray(n * row_len_ * sizeof(float));
  kern::SparseGatherF32(reinterpret_cast<const float*>(table_.data()), rows, n, row_len_,
                        reinterpret_cast<float*>(out.data()), stream, key_shift_, row_base_, rows_);
  KVPairs<float> res;
  // keys stay meta-only: device keys must not be dereferenced host-side
  res.vals = SArray<float>::View(out);
  SArray<int> lens(1);
  lens[0] = static_cast<int>(n * row_len_);
  res.lens = lens;
  // drained whenever no destination was advertised; the dense handlers'
  // HbmDest also drains for a host-pool destination
  if (!(req.option & kOptPullAddr)) XPS_HIP_CHECK(hipStreamSynchronize(stream));
  server->Response(req, res);
}

void GpuSparseHandler::operator()(const KVMeta& req, const KVPairs<float>& kvs,
                                  KVServer<float>* server) {
  XPS_HIP_CHECK(hipSetDevice(HbmPool::Get()->device()));
  hipStream_t stream = Stream(req.sender);
  size_t n = kvs.keys.size();
  XPS_CHECK_GT(n, 0u);
  float* table = reinterpret_cast<float*>(table_.data());
  if (req.push) {
    XPS_CHECK(kvs.vals.on_device()) << "sparse push needs device vals (pool buffers)";
    XPS_CHECK_EQ(kvs.vals.size(), n * row_len_);
    const uint64_t* rows = DeviceKeys(kvs.keys, req.sender, stream);
    if (accumulate_ || req.cmd == kCmdSum) {
      kern::SparseScatterAddF32(table, rows, n, row_len_, kvs.vals.data(), atomic_,
                                stream, key_shift_, row_base_, rows_);
    } else {
      kern::SparseScatterAssignF32(table, rows, n, row_len_, kvs.vals.data(), stream, key_shift_,
                                   row_base_, rows_);
    }
    if (req.pull) {
      // fused round (ZPushPull): gather the post-scatter rows on the
      // SAME stream (ordered behind the scatter) and answer in one trip
      GatherRespond(req, rows, n, stream, server);
      return;
    }
    if (!ThePlane(po_)) XPS_HIP_CHECK(hipStreamSynchronize(stream));
    server->Response(req);
  } else if (req.pull) {
    GatherRespond(req, DeviceKeys(kvs.keys, req.sender, stream), n, stream, server);
  }
}

void GpuSparseHandler::Save(const std::string& path) {
  FILE* f = fopen(path.c_str(), "wb");
  XPS_CHECK(f) << "cannot open checkpoint " << path;
  uint64_t hdr[3] = {rows_, row_len_, static_cast<uint64_t>(key_shift_)};
  fwrite(hdr, 8, 3, f);
  std::vector<char> host(table_.size());
  XPS_HIP_CHECK(hipMemcpy(host.data(), table_.data(), table_.size(), hipMemcpyDeviceToHost));
  fwrite(host.data(), 1, host.size(), f);
  fclose(f);
}

void GpuSparseHandler::Load(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  XPS_CHECK(f) << "cannot open checkpoint " << path;
  uint64_t hdr[3];
  XPS_CHECK_EQ(fread(hdr, 8, 3, f), 3u);
  XPS_CHECK_EQ(hdr[0], rows_);
  XPS_CHECK_EQ(hdr[1], row_len_);
  std::vector<char> host(table_.size());
  XPS_CHECK_EQ(fread(host.data(), 1, host.size(), f), host.size());
  XPS_HIP_CHECK(hipMemcpy(table_.data(), host.data(), table_.size(), hipMemcpyHostToDevice));
  fclose(f);
}

}  // namespace xps
