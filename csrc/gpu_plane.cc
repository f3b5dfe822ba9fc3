#include "gpu_plane.h"

#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <semaphore.h>
#include <sys/prctl.h>
#include <time.h>
#include <unistd.h>

#include <cstring>

#include "hip_check.h"
#include "hip_pool.h"
#include "host_par.h"
#include "host_pool.h"
#include "kernels.h"
#include "postoffice.h"
#include "wire.h"

namespace xps {

static const size_t kInlineMax = 4096;  // host blobs above this ride the shm pool

// count of blobs received BY REFERENCE (pool offset, no copy) — the
// zero-copy assertion hook (reference test_benchmark.cc:169-181 checks
// pointer equality against registered buffers; here the transport
// itself reports it)
std::atomic<uint64_t> g_zero_copy_recv{0};
std::atomic<uint64_t> g_fused_assign{0};

bool FusedAssignEnabled() {
  static const bool on = Environment::Get()->GetInt("XPS_FUSED_ASSIGN", 1) != 0;
  return on;
}

std::atomic<uint64_t> g_fused_launches{0};

bool CoalesceEnabled() {
  static const bool on = Environment::Get()->GetInt("XPS_COALESCE", 1) != 0;
  return on;
}

namespace {
// CoalesceAppend's hand-over to the deferred response that the same
// thread sends next (handler -> KVServer::Response -> Send)
struct CoTicket {
  const void* plane = nullptr;
  int peer = 0;
  std::shared_ptr<void> cev;
};
thread_local CoTicket t_co_ticket;

int64_t NowUs() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return static_cast<int64_t>(ts.tv_sec) * 1000000 + ts.tv_nsec / 1000;
}
// XPS_COALESCE_HOLD: the completion thread launches a held batch once no
// key joined it for this long (a burst appends every few microseconds)
const int64_t kHoldQuietUs = 2000;
// in-flight payload below which a stream does not count as busy: about
// 8 us of dual-write traffic at the 5.8 TB/s the kernel sustains
const size_t kCoBusyBytes = 16u << 20;

// process-wide dedup of hipIpcOpenMemHandle (two vans of a joint process
// and multiple planes share peer pool mappings; never closed — pools are
// process-lifetime)
std::mutex g_map_mu;
struct HandleKey {
  char h[kIpcHandleBytes];
  bool operator==(const HandleKey& o) const { return memcmp(h, o.h, kIpcHandleBytes) == 0; }
};
struct HandleHash {
  size_t operator()(const HandleKey& k) const {
    size_t v = 1469598103934665603ull;
    for (char c : k.h) {
      v ^= static_cast<unsigned char>(c);
      v *= 1099511628211ull;
    }
    return v;
  }
};
std::unordered_map<HandleKey, void*, HandleHash> g_mapped;

// Host-wide lock around hipIpcOpenMemHandle. Two processes importing
// each other's pools CONCURRENTLY deadlock inside the HIP runtime
// (measured on ROCm 7.x: the import handshake needs the exporter's
// runtime lock, held by its own in-flight import — cross-process AB-BA).
// Serializing imports host-wide breaks the cycle.
class IpcOpenLock {
 public:
  IpcOpenLock() {
    sem_ = sem_open("/xps_ipc_open_lock", O_CREAT, 0600, 1);
  }
  void Lock() {
    if (sem_ == SEM_FAILED) return;
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    ts.tv_sec += 60;
    if (sem_timedwait(sem_, &ts) != 0) {
      XPS_LOG(Warning) << "ipc-open lock timeout; proceeding unlocked";
      timed_out_ = true;
    }
  }
  void Unlock() {
    if (sem_ != SEM_FAILED && !timed_out_) sem_post(sem_);
    timed_out_ = false;
  }

 private:
  sem_t* sem_ = SEM_FAILED;
  bool timed_out_ = false;
};
IpcOpenLock g_ipc_lock;
}  // namespace

GpuPlane::GpuPlane(Postoffice* po, int device) : po_(po), device_(device) {
  my_host_hash_ = HostHash();
  inline_deliver_ = Environment::Get()->GetInt("XPS_INLINE_HANDLER", 1) != 0;
  lanes_ = Environment::Get()->GetInt("XPS_STREAMS_PER_PEER", 2);
  if (lanes_ < 1) lanes_ = 1;
  if (lanes_ > 2) lanes_ = 2;
  co_hold_ = Environment::Get()->GetInt("XPS_COALESCE_HOLD", 0) != 0;
  int cap_mb = Environment::Get()->GetInt("XPS_COALESCE_CAP_MB", 1024);
  co_byte_cap_ = static_cast<size_t>(cap_mb < 1 ? 1 : cap_mb) << 20;
}

GpuPlane::~GpuPlane() { Stop(); }

void GpuPlane::FillSelf(Node* self) {
  // reap segments left by crashed/killed runs before creating ours
  static std::once_flag gc_once;
  std::call_once(gc_once, [] { HostShmPool::GcStaleSegments(); });
  self->dev_id = device_;
  auto* pool = HbmPool::Get();
  if (device_ >= 0 && pool->initialized()) {
    self->pool_capacity = pool->capacity();
    self->pool_slab_bytes = pool->slab_bytes();
    self->pool_handles.resize(pool->slab_count());
    for (size_t i = 0; i < pool->slab_count(); ++i) {
      memcpy(self->pool_handles[i].data(), pool->slab_handle(i), kIpcHandleBytes);
    }
  }
  // host-shm arena: zero-copy HOST payloads for same-host peers (one per
  // process; both nodes of a joint process advertise the same uid)
  auto* hpool = HostShmPool::Get();
  hpool->Init(self->shm_uid);
  self->host_pool_uid = hpool->uid();
  self->host_pool_capacity = hpool->capacity();
  if (!started_) {
    auto* env = Environment::Get();
    if (!env->GetInt("XPS_PROBE_NO_RING", 0)) {
      XPS_CHECK(in_ring_.Create(self->shm_uid)) << "cannot create shm ring";
    }
    started_ = true;
    if (!env->GetInt("XPS_PROBE_NO_POLL", 0)) {
      poll_running_ = true;
      poll_thread_ = std::thread([this] { RingPollLoop(); });
    }
    if (device_ >= 0 && !env->GetInt("XPS_PROBE_NO_COMP", 0)) {
      comp_thread_ = std::thread([this] { CompletionLoop(); });
    }
  }
}

void GpuPlane::Stop() {
  if (stop_.exchange(true)) return;
  PrintStageStats(device_ >= 0 ? "gpu plane" : "host plane");
  if (poll_thread_.joinable()) poll_thread_.join();
  if (comp_thread_.joinable()) comp_thread_.join();
  // deliver any same-process messages the poll thread didn't get to
  // (customers are still alive: the van stops after its plane)
  {
    std::lock_guard<std::mutex> lk(local_mu_);
    for (auto& lm : local_q_) po_->van()->Deliver(std::move(lm.first));
    local_q_.clear();
  }
  // launch whatever the coalescer still holds, then drop its event refs
  // (they return to the event pool, which goes below)
  if (device_ >= 0) {
    std::vector<Peer*> all;
    {
      std::shared_lock<std::shared_timed_mutex> lk(peers_mu_);
      for (auto& kv : peers_) all.push_back(kv.second.get());
    }
    for (Peer* peer : all) {
      CoFlush(peer);
      std::lock_guard<std::mutex> lk(peer->co.mu);
      peer->co.inflight.clear();
    }
  }
  // drain pending sends synchronously so responses are not lost on stop
  {
    std::lock_guard<std::mutex> lk(pend_mu_);
    for (auto& kv : pending_) {
      for (auto& p : kv.second) {
        if (p.cev) {
          // shared event of a coalesced launch: wait, never destroy here
          // (its siblings still hold it; the last one pools it)
          (void)hipEventSynchronize(p.cev->ev.load(std::memory_order_acquire));
          if (p.local_po) {
            DeliverLocal(p.local_po, p.resend, p.bytes);
          } else {
            Peer* peer = GetPeer(p.peer_id);
            auto ring = peer ? RingOf(peer) : nullptr;
            if (!ring || !ring->Push(p.payload.data(),
                                     static_cast<uint32_t>(p.payload.size()))) {
              (void)po_->van()->SendOverTcp(p.resend, p.peer_id);
            }
          }
          continue;
        }
        (void)hipEventSynchronize(p.ev);
        if (p.local_po) {
          DeliverLocal(p.local_po, p.resend, p.bytes);
          (void)hipEventDestroy(p.ev);
          continue;
        }
        Peer* peer = GetPeer(p.peer_id);
        auto ring = peer ? RingOf(peer) : nullptr;
        bool sent = ring && ring->Push(p.payload.data(),
                                       static_cast<uint32_t>(p.payload.size()));
        if (!sent) {
          // van TCP conns are still open (plane stops first): best-effort
          (void)po_->van()->SendOverTcp(p.resend, p.peer_id);
        }
        (void)hipEventDestroy(p.ev);
      }
    }
    pending_.clear();
  }
  in_ring_.CloseAndUnlink();
  HostShmPool::Get()->Unlink();  // idempotent; mappings stay valid
  std::lock_guard<std::mutex> lk(ev_mu_);
  for (auto ev : event_pool_) (void)hipEventDestroy(ev);
  event_pool_.clear();
}

void GpuPlane::OnPeer(const Node& peer) {
  if (peer.host_hash != my_host_hash_) return;
  std::unique_lock<std::shared_timed_mutex> lk(peers_mu_);
  auto& p = peers_[peer.id];
  if (!p) p.reset(new Peer());
  if (p->node.shm_uid != 0 && peer.shm_uid != 0 && p->node.shm_uid != peer.shm_uid) {
    // RECOVERY: the id now names a NEW process. Every cached resource
    // of the old one is stale — the ring segment has no consumer, the
    // slab mappings point at a dead process's pool (writing through
    // them would corrupt whatever reused that memory), and local_po may
    // name the wrong instance. Reset; the next send re-opens/re-imports
    // lazily. The old ring object stays alive via shared_ptr for any
    // in-flight push.
    std::lock_guard<std::mutex> lk2(p->mu);
    XPS_LOG(Warning) << "peer " << peer.id << " was recovered (new process); resetting "
                        "plane caches for it";
    p->ring_ok.store(false, std::memory_order_release);
    p->ring_tried = false;
    std::atomic_store_explicit(&p->ring, std::shared_ptr<ShmRing>(),
                               std::memory_order_release);
    p->pool_tried = false;
    p->slab_bases.clear();
    p->local_po.store(nullptr, std::memory_order_release);
  }
  p->node = peer;
}

void GpuPlane::ImportPeers() {
  // collect ids first (don't hold peers_mu_ across the import)
  std::vector<int> ids;
  {
    std::shared_lock<std::shared_timed_mutex> lk(peers_mu_);
    for (auto& kv : peers_) ids.push_back(kv.first);
  }
  for (int id : ids) {
    Peer* p = GetPeer(id);
    if (p->node.pool_capacity) {
      bool ok = ImportPeerSlabs(p);
      XPS_VLOG(1) << "imported pool of peer " << id << " (" << p->node.pool_handles.size()
                  << " slabs): " << (ok ? "ok" : "FAILED");
    }
  }
}

GpuPlane::Peer* GpuPlane::GetPeer(int id) {
  {
    std::shared_lock<std::shared_timed_mutex> lk(peers_mu_);
    auto it = peers_.find(id);
    if (it != peers_.end()) return it->second.get();
  }
  std::unique_lock<std::shared_timed_mutex> lk(peers_mu_);
  auto& p = peers_[id];
  if (!p) {
    p.reset(new Peer());
    p->node = po_->van()->GetNode(id);
  }
  return p.get();
}

bool GpuPlane::EnsureRing(Peer* p) {
  if (p->ring_ok.load(std::memory_order_acquire)) return true;
  std::lock_guard<std::mutex> lk(p->mu);
  {
    auto cur = std::atomic_load_explicit(&p->ring, std::memory_order_acquire);
    if (cur && cur->ok()) return true;
  }
  if (p->ring_tried) return false;
  p->ring_tried = true;
  if (p->node.shm_uid == 0) return false;
  auto ring = std::make_shared<ShmRing>();
  if (!ring->Open(p->node.shm_uid)) return false;
  std::atomic_store_explicit(&p->ring, std::shared_ptr<ShmRing>(std::move(ring)),
                             std::memory_order_release);
  p->ring_ok.store(true, std::memory_order_release);
  return true;
}

std::shared_ptr<ShmRing> GpuPlane::RingOf(Peer* p) {
  if (!EnsureRing(p)) return nullptr;
  // lock-free snapshot: the recovery path swaps the pointer with
  // atomic_store, so the hot send path never takes p->mu
  return std::atomic_load_explicit(&p->ring, std::memory_order_acquire);
}

bool GpuPlane::ImportPeerSlabs(Peer* p) {
  {
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->pool_tried) return !p->slab_bases.empty();
    p->pool_tried = true;
  }
  std::vector<void*> bases;
  auto* pool = HbmPool::Get();
  size_t nslabs = p->node.pool_handles.size();
  bool same_process =
      pool->initialized() && nslabs == pool->slab_count() &&
      memcmp(p->node.pool_handles[0].data(), pool->slab_handle(0), kIpcHandleBytes) == 0;
  // Cross-DEVICE import: our kernels will load/store the mapping over
  // xGMI, which needs peer access from our device to the exporter's.
  // Enable it eagerly at bootstrap — a lazy failure would surface as a
  // memory fault inside a steady-state kernel. peer dev_id is the peer
  // PROCESS's device index; it translates directly when all ranks see
  // the same HIP_VISIBLE_DEVICES ordering (the one-proc-per-GPU layout).
  int peer_dev = p->node.dev_id;
  if (!same_process && peer_dev >= 0 && peer_dev != device_ &&
      Environment::Get()->GetInt("XPS_PEER_ACCESS_CHECK", 1)) {
    int ndev = 0;
    (void)hipGetDeviceCount(&ndev);
    if (peer_dev < ndev) {
      int can = 0;
      (void)hipDeviceCanAccessPeer(&can, device_, peer_dev);
      if (!can) {
        XPS_LOG(Warning) << "device " << device_ << " cannot peer-access device " << peer_dev
                         << " (peer node " << p->node.id
                         << "): keeping this peer on the TCP path";
        std::lock_guard<std::mutex> lk(p->mu);
        p->slab_bases.clear();
        return false;
      }
      XPS_HIP_CHECK(hipSetDevice(device_));
      hipError_t pe = hipDeviceEnablePeerAccess(peer_dev, 0);
      if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) {
        XPS_LOG(Warning) << "hipDeviceEnablePeerAccess(" << peer_dev
                         << ") failed: " << hipGetErrorString(pe)
                         << " (continuing; hipIpc lazy enable may still cover it)";
      }
    }
  }
  for (size_t i = 0; i < nslabs; ++i) {
    void* base = nullptr;
    if (same_process) {
      base = pool->slab_base(i);  // joint process: use the local mapping
    } else {
      HandleKey key;
      memcpy(key.h, p->node.pool_handles[i].data(), kIpcHandleBytes);
      std::lock_guard<std::mutex> lk(g_map_mu);
      auto it = g_mapped.find(key);
      if (it != g_mapped.end()) {
        base = it->second;
      } else {
        XPS_HIP_CHECK(hipSetDevice(device_));
        hipIpcMemHandle_t h;
        memcpy(&h, p->node.pool_handles[i].data(), sizeof(h));
        XPS_VLOG(3) << "ipc-open slab " << i << " of peer " << p->node.id;
        g_ipc_lock.Lock();
        hipError_t e = hipIpcOpenMemHandle(&base, h, hipIpcMemLazyEnablePeerAccess);
        g_ipc_lock.Unlock();
        XPS_VLOG(3) << "ipc-open slab " << i << " of peer " << p->node.id << " -> " << base;
        if (e != hipSuccess) {
          XPS_LOG(Warning) << "hipIpcOpenMemHandle(peer " << p->node.id << " slab " << i
                           << ") failed: " << hipGetErrorString(e)
                           << " — peer stays on the TCP path";
          base = nullptr;
        } else {
          // probe the mapping NOW (one 8-byte D2H read): a dead or
          // access-less mapping must fail loudly at bootstrap, not as a
          // memory fault inside a steady-state kernel
          char probe[8];
          hipError_t e2 = hipMemcpy(probe, base, sizeof(probe), hipMemcpyDeviceToHost);
          if (e2 != hipSuccess) {
            XPS_LOG(Warning) << "peer " << p->node.id << " slab " << i
                             << " mapped but unreadable (" << hipGetErrorString(e2)
                             << ") — peer stays on the TCP path";
            base = nullptr;
          }
        }
        g_mapped[key] = base;
      }
    }
    if (!base) {
      std::lock_guard<std::mutex> lk(p->mu);
      p->slab_bases.clear();
      return false;
    }
    bases.push_back(base);
  }
  std::lock_guard<std::mutex> lk(p->mu);
  p->slab_bases = std::move(bases);
  return !p->slab_bases.empty();
}

char* GpuPlane::ResolvePeer(Peer* p, uint64_t global_off, uint64_t len) {
  if (!ImportPeerSlabs(p)) return nullptr;
  uint64_t slab_bytes = p->node.pool_slab_bytes;
  if (slab_bytes == 0) return nullptr;
  size_t idx = static_cast<size_t>(global_off / slab_bytes);
  uint64_t local = global_off % slab_bytes;
  std::lock_guard<std::mutex> lk(p->mu);
  // compare against the remaining room, never local + len (which can
  // wrap for a hostile/corrupt length)
  if (idx >= p->slab_bases.size() || len > slab_bytes - local) {
    XPS_LOG(Warning) << "peer offset out of bounds: off=" << global_off << " len=" << len
                     << " slab=" << idx;
    return nullptr;
  }
  return static_cast<char*>(p->slab_bases[idx]) + local;
}

hipStream_t GpuPlane::StreamLane(int node_id, int lane) {
  if (lane >= lanes_) lane = lanes_ - 1;
  Peer* p = GetPeer(node_id);
  if (lane == 0) CoFlush(p);
  return RawLane(p, lane);
}

bool GpuPlane::LanesSplit(int node_id) {
  return lanes_ >= 2 && GetPeer(node_id)->node.dev_id != device_;
}

// ---- dual-write launch coalescer ------------------------------------------

void GpuPlane::CoLaunchLocked(Peer* p) {
  Coalescer& co = p->co;
  if (co.n == 0) return;
  hipStream_t stream = RawLane(p, 0);
  XPS_HIP_CHECK(hipSetDevice(device_));
  if (co.n == 1) {
    const kern::Seg2& s = co.segs[0];
    kern::DenseAssign2(s.dst0, s.dst1, s.src, s.nbytes, stream);
  } else {
    kern::BatchedAssign2(co.segs, co.n, stream);
  }
  g_fused_launches.fetch_add(1, std::memory_order_relaxed);
  hipEvent_t ev = GetEvent();
  XPS_HIP_CHECK(hipEventRecord(ev, stream));
  co.open->bytes = co.bytes;
  co.open->ev.store(ev, std::memory_order_release);
  co.inflight.push_back(std::move(co.open));
  co.open.reset();
  co.n = 0;
  co.bytes = 0;
  co.n_open.store(0, std::memory_order_release);
}

// Is the GPU the bottleneck of this stream? Two coalesced launches still
// in flight AND enough bytes in them to outlast a launch: 2 x 1 MiB drain
// in about a microsecond, so holding small keys back only adds a hop
// (measured on the 1 MiB per-key config, see the profile file).
bool GpuPlane::CoBusyLocked(Peer* p) {
  CoPruneLocked(p);
  size_t bytes = 0;
  for (auto& f : p->co.inflight) bytes += f->bytes;
  return p->co.inflight.size() >= 2 && bytes >= kCoBusyBytes;
}

void GpuPlane::CoPruneLocked(Peer* p) {
  auto& fl = p->co.inflight;
  while (!fl.empty()) {
    CoEvent* f = fl.front().get();
    if (!f->done.load(std::memory_order_acquire) &&
        hipEventQuery(f->ev.load(std::memory_order_acquire)) != hipSuccess) {
      break;
    }
    fl.pop_front();
  }
}

void GpuPlane::CoFlush(Peer* p) {
  if (p->co.n_open.load(std::memory_order_acquire) == 0) return;
  std::lock_guard<std::mutex> lk(p->co.mu);
  CoLaunchLocked(p);
}

std::shared_ptr<GpuPlane::CoEvent> GpuPlane::CoAppend(Peer* p, const kern::Seg2& seg) {
  if (!CoalesceEnabled()) return nullptr;
  Coalescer& co = p->co;
  std::lock_guard<std::mutex> lk(co.mu);
  kern::Admit a = kern::CoalesceAdmit(co.segs, co.n, seg);
  if (a != kern::Admit::kAdmit) CoLaunchLocked(p);
  if (a == kern::Admit::kReject) return nullptr;
  if (!co.open) co.open = std::make_shared<CoEvent>(this);
  std::shared_ptr<CoEvent> cev = co.open;
  co.segs[co.n++] = seg;
  co.bytes += seg.nbytes;
  co.n_open.store(co.n, std::memory_order_release);
  if (co.n >= kern::kMaxBatch || co.bytes >= co_byte_cap_) {
    CoLaunchLocked(p);
  } else if (co_hold_) {
    co.last_append_us = NowUs();
  } else {
    // an idle GPU gets the key at once; a busy one keeps exactly one
    // launch queued behind the running one and lets the rest pile up
    if (!CoBusyLocked(p)) CoLaunchLocked(p);
  }
  return cev;
}

bool GpuPlane::CoFrontUnlaunched(Peer* p, const std::shared_ptr<CoEvent>& cev) {
  Coalescer& co = p->co;
  std::lock_guard<std::mutex> lk(co.mu);
  if (co.open != cev) return true;  // launched meanwhile
  if (co_hold_ && NowUs() - co.last_append_us < kHoldQuietUs) return false;
  CoLaunchLocked(p);
  return true;
}

void GpuPlane::CoRetired(Peer* p) {
  Coalescer& co = p->co;
  std::lock_guard<std::mutex> lk(co.mu);
  bool busy = CoBusyLocked(p);
  if (!co_hold_ && !busy) CoLaunchLocked(p);
}

bool GpuPlane::CoalesceAppend(int peer_id, const kern::Seg2& seg) {
  if (device_ < 0) return false;
  std::shared_ptr<CoEvent> cev = CoAppend(GetPeer(peer_id), seg);
  if (!cev) return false;
  t_co_ticket.plane = this;
  t_co_ticket.peer = peer_id;
  t_co_ticket.cev = std::move(cev);
  return true;
}

std::shared_ptr<GpuPlane::CoEvent> GpuPlane::TakeTicket(int peer_id) {
  if (!t_co_ticket.cev || t_co_ticket.plane != this || t_co_ticket.peer != peer_id) {
    return nullptr;
  }
  auto cev = std::static_pointer_cast<CoEvent>(t_co_ticket.cev);
  t_co_ticket.cev.reset();
  return cev;
}

void GpuPlane::CoalesceEnd(int peer_id) {
  if (!t_co_ticket.cev) return;  // a deferred response took the batch's event
  t_co_ticket.cev.reset();
  CoFlush(GetPeer(peer_id));
}

hipStream_t GpuPlane::RawLane(Peer* p, int lane) {
  hipStream_t s = p->streams[lane].load(std::memory_order_acquire);
  if (s) return s;
  std::lock_guard<std::mutex> lk(p->mu);
  s = p->streams[lane].load(std::memory_order_relaxed);
  if (!s) {
    XPS_HIP_CHECK(hipSetDevice(device_));
    XPS_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    p->streams[lane].store(s, std::memory_order_release);
  }
  return s;
}

hipStream_t GpuPlane::StreamForPeer(int node_id) { return StreamLane(node_id, 0); }

hipStream_t GpuPlane::PullStreamForPeer(int node_id) {
  // The pull lane pays only CROSS-device: push kernels (reads from the
  // peer over xGMI) and pull copies (writes to the peer) then use the
  // link full duplex. Same-device peers share HBM, so a second lane
  // adds chain events without adding bandwidth (measured -11% on the
  // 64 MB same-GPU config) — collapse to lane 0.
  Peer* p = GetPeer(node_id);
  if (lanes_ < 2 || p->node.dev_id == device_) return StreamLane(node_id, 0);
  CoFlush(p);  // pull-lane work is chained behind lane 0 by events recorded there
  return StreamLane(node_id, 1);
}

std::vector<std::tuple<int, int64_t, int64_t>> GpuPlane::PeerBytes() {
  std::vector<std::tuple<int, int64_t, int64_t>> out;
  std::shared_lock<std::shared_timed_mutex> lk(peers_mu_);
  for (auto& kv : peers_) {
    int64_t tx = kv.second->tx_bytes.load(std::memory_order_relaxed);
    int64_t rx = kv.second->rx_bytes.load(std::memory_order_relaxed);
    if (tx || rx) out.emplace_back(kv.first, tx, rx);
  }
  return out;
}

hipEvent_t GpuPlane::GetEvent() {
  {
    std::lock_guard<std::mutex> lk(ev_mu_);
    if (!event_pool_.empty()) {
      hipEvent_t ev = event_pool_.back();
      event_pool_.pop_back();
      return ev;
    }
  }
  hipEvent_t ev;
  XPS_HIP_CHECK(hipSetDevice(device_));
  XPS_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  return ev;
}

void GpuPlane::PutEvent(hipEvent_t ev) {
  std::lock_guard<std::mutex> lk(ev_mu_);
  event_pool_.push_back(ev);
}

Postoffice* GpuPlane::LocalPeer(Peer* p) {
  Postoffice* po = p->local_po.load(std::memory_order_acquire);
  if (po) return po;
  if (p->node.id == kEmptyNodeID) return nullptr;
  po = Postoffice::FindByNodeId(p->node.id);
  if (po) p->local_po.store(po, std::memory_order_release);
  return po;
}

// ack of a one-sided push, or of a one-sided fused push+pull (its
// response keeps the request's kOptEntryPush; the handler's own fused
// launch clears it): the handler launched nothing, so there is no event
// to wait for
static bool KernelLessAck(const Message& msg) {
  return !msg.meta.request && msg.meta.push && (msg.meta.option & kOptInPlace) &&
         (!msg.meta.pull || (msg.meta.option & kOptEntryPush));
}

// does this (device-vals) pull response REQUIRE the staging path? The
// worker-side merge expects host bytes unless an in-place HBM
// destination was advertised.
static bool NeedsStaging(const Message& msg) {
  return !msg.meta.request && msg.meta.pull && msg.data.size() > 1 &&
         msg.data[1].on_device() && msg.data[1].size() > 0 &&
         (!(msg.meta.option & kOptPullAddr) || (msg.meta.option & kOptHostAddr));
}

// pull response whose requester advertised where the values go ...
static bool HasPullDest(const Message& msg) {
  return !msg.meta.request && msg.meta.pull && msg.data.size() > 1 &&
         (msg.meta.option & kOptPullAddr);
}
// ... HOST vals for a destination in its host pool
static bool HostDest(const Message& msg) {
  return (msg.meta.option & kOptHostAddr) && !msg.data[1].on_device() && msg.data[1].size() > 0;
}
// ... device vals for a destination in its HBM pool
static bool HbmDest(const Message& msg) {
  return !(msg.meta.option & kOptHostAddr) && msg.data[1].on_device();
}

// The synchronous-handler contract: a host handler's response may be a
// VIEW of mutable server state, and the store may mutate right after
// Response returns. The wire paths serialize before that; a same-process
// delivery takes a private copy instead.
static SArray<char> Snapshot(const SArray<char>& d) {
  SArray<char> copy(d.size());
  memcpy(copy.data(), d.data(), d.size());
  return copy;
}

// what an in-place note does with the host blobs it keeps
enum class NoteBlobs {
  kShare,       // same buffers as msg
  kSnapshot,    // private copies (see Snapshot)
  kInlineOnly,  // shared, minus blobs over kInlineMax: the note must fit the ring
};

// The meta-only message that follows an in-place write of msg's vals
// (blob 1): msg's meta with kOptInPlace and val_len set, plus msg's host
// blobs other than blob 1 (keys/lens for the merge bookkeeping), with
// data_type rebuilt to match.
static Message InPlaceNote(const Message& msg, size_t val_len,
                           NoteBlobs how = NoteBlobs::kShare) {
  Message note;
  note.meta = msg.meta;
  note.meta.option |= kOptInPlace;
  note.meta.val_len = static_cast<int64_t>(val_len);
  note.meta.data_type.clear();
  for (size_t i = 0; i < msg.data.size(); ++i) {
    const SArray<char>& d = msg.data[i];
    if (i == 1 || d.on_device()) continue;
    if (how == NoteBlobs::kInlineOnly && d.size() > kInlineMax) continue;
    note.data.push_back(how == NoteBlobs::kSnapshot ? Snapshot(d) : d);
    note.meta.data_type.push_back(msg.meta.data_type[i]);
  }
  return note;
}

// the vals of an in-place write stay alive until its event fires
static Message KeepAlive(const SArray<char>& vals) {
  Message keepalive;
  keepalive.data.push_back(vals);
  return keepalive;
}

static GpuPlane* PlaneOf(Postoffice* po) {
  return dynamic_cast<GpuPlane*>(po->van() ? po->van()->plane() : nullptr);
}

// XPS_LOCAL_QUEUE_REQ=1: same-process requests are queued to the
// receiver's poll thread instead of delivered inline
static bool LocalQueueReq() {
  static const bool on = Environment::Get()->GetInt("XPS_LOCAL_QUEUE_REQ", 0) != 0;
  return on;
}

bool GpuPlane::CanSend(const Message& msg, const Node& peer) {
  if (!started_ || stop_.load()) return false;
  if (peer.host_hash != my_host_hash_ || peer.shm_uid == 0) return false;
  // same-process peer (joint mode): everything rides the direct path —
  // no ring-size limits, no pool-membership requirement (one address
  // space) — except responses that need the TCP host-staging contract
  if (LocalPeer(GetPeer(peer.id))) return !NeedsStaging(msg);
  // If the bootstrap import of this peer's pool failed, assume the
  // reverse import failed too (same mechanism, same host) and keep
  // everything on the TCP path — slow but never dropped.
  if (peer.pool_capacity) {
    Peer* p = GetPeer(peer.id);
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->pool_tried && p->slab_bases.empty()) return false;
  }
  size_t est = 160 + msg.meta.body.size();
  for (size_t i = 0; i < msg.data.size(); ++i) {
    const auto& d = msg.data[i];
    if (d.on_device()) {
      uint64_t off;
      if (!HbmPool::Get()->OffsetOf(d.data(), &off)) return false;  // not our pool -> TCP
      est += 24;
      // device vals in a pull response need an HBM in-place destination
      if (!msg.meta.request && msg.meta.pull && i == 1) {
        if (!(msg.meta.option & kOptPullAddr) || (msg.meta.option & kOptHostAddr) ||
            peer.pool_capacity == 0) {
          return false;
        }
      }
    } else if (d.size() > kInlineMax) {
      uint64_t off;
      if (!HostShmPool::Get()->OffsetOf(d.data(), &off)) return false;  // big + unpooled -> TCP
      est += 24;
    } else {
      est += 24 + d.size();
    }
  }
  return est <= ShmRing::MaxPayload();
}

bool GpuPlane::Serialize(const Message& msg, const std::vector<char>& by_ref, std::string* out) {
  XPS_STAGE(serialize);
  std::string meta;
  PackMeta(msg.meta, &meta);
  out->clear();
  out->reserve(meta.size() + 64);
  ByteWriter w(out);
  w.U64(meta.size());
  w.Raw(meta.data(), meta.size());
  w.U8(static_cast<uint8_t>(msg.data.size()));
  for (size_t i = 0; i < msg.data.size(); ++i) {
    const auto& d = msg.data[i];
    if (by_ref[i] == 1) {  // HBM pool ref
      uint64_t off = 0;
      XPS_CHECK(HbmPool::Get()->OffsetOf(d.data(), &off));
      w.U8(1);
      w.U64(off);
      w.U64(d.size());
    } else if (by_ref[i] == 2) {  // host shm pool ref
      uint64_t off = 0;
      XPS_CHECK(HostShmPool::Get()->OffsetOf(d.data(), &off));
      w.U8(2);
      w.U64(off);
      w.U64(d.size());
    } else {
      w.U8(0);
      w.U64(d.size());
      w.Raw(d.data(), d.size());
    }
  }
  return out->size() <= ShmRing::MaxPayload();
}

void GpuPlane::DeliverLocal(Postoffice* lpo, Message& msg, int64_t bytes) {
  Van* van = lpo->van();
  if (!van) {
    XPS_LOG(Warning) << "local peer " << msg.meta.recver << " already finalized; dropping";
    return;
  }
  auto* rplane = dynamic_cast<GpuPlane*>(van->plane());
  // In-handler sends must be queued to the receiver's poll thread:
  // delivering them inline would nest two customers' handle_mu_ in the
  // opposite order of the worker-callback -> request chain (see
  // customer.cc). Requests deliver inline by default (lowest latency —
  // measured better than queue-pipelining for single-flow traffic);
  // XPS_LOCAL_QUEUE_REQ=1 opts into the queued/pipelined variant.
  if (InCustomerHandler() || (LocalQueueReq() && msg.meta.request)) {
    if (rplane && rplane->poll_running_) {
      rplane->EnqueueLocal(std::move(msg), bytes);
      return;
    }
    XPS_CHECK(!InCustomerHandler())
        << "in-handler local send needs the receiver's poll thread";
  }
  HandToVan(van, msg, bytes, true);
}

void GpuPlane::HandToVan(Van* van, Message& msg, int64_t bytes, bool count_refs) {
  van->recv_bytes_ += bytes;
  // blobs handed over by reference in one address space = zero-copy
  // reception (the transport-level analog of the reference's
  // registered-buffer pointer-equality assertion). The ring path counts
  // its own while it resolves them.
  if (count_refs) {
    for (auto& d : msg.data) {
      if (d.size() && (d.on_device() || d.size() > kInlineMax)) {
        g_zero_copy_recv.fetch_add(1, std::memory_order_relaxed);
      }
    }
  }
  if (inline_deliver_) {
    van->DeliverInline(msg);
  } else {
    van->Deliver(std::move(msg));
  }
}

GpuPlane* GpuPlane::OneSidedOwner(Peer* p, Postoffice** elpo) {
  *elpo = LocalPeer(p);
  if (!*elpo) return EnsureRing(p) ? this : nullptr;
  // Cross-process the one-sided write removes the server-side launch
  // entirely (2012 -> 2603 GB/s on the 2-joint-procs-1-GPU config). For a
  // SAME-process peer it is measured SLOWER (61 vs 84 GB/s per-key 1 MB,
  // RTT 50 vs 42 us, same-box A/B: the app thread becomes the single
  // launch lane) — default off locally; XPS_LOCAL_ONE_SIDED=1 re-enables
  // it (the write then runs on the RECEIVER plane's stream for us, so
  // ordering stays stream-based).
  static const bool local_one_sided =
      Environment::Get()->GetInt("XPS_LOCAL_ONE_SIDED", 0) != 0;
  return local_one_sided ? PlaneOf(*elpo) : nullptr;
}

hipStream_t GpuPlane::OneSidedLane(GpuPlane* owner, Peer* p) {
  return owner == this ? StreamForPeer(p->node.id) : owner->StreamForPeer(po_->node_id());
}

bool GpuPlane::LocalPullRead(int peer_id, void* dst, uint64_t entry_off, size_t len,
                             Message resp) {
  if (device_ < 0 || !started_ || stop_.load()) return false;
  Peer* p = GetPeer(peer_id);
  char* src = ResolvePeer(p, entry_off, len);
  if (!src) return false;
  XPS_STAGE(local_pull_read);
  // lane 0 of the stream our entry pushes used: for a same-process peer
  // that is the RECEIVER plane's stream for us (also the stream its
  // handler kernels run on), else our own per-peer stream. Not
  // OneSidedOwner's rule: a read needs neither XPS_LOCAL_ONE_SIDED nor
  // the peer's ring, and has a condition of its own.
  GpuPlane* owner = this;
  if (Postoffice* elpo = LocalPeer(p)) {
    owner = PlaneOf(elpo);
    if (!owner) return false;
    // ordering relies on the preceding LOCAL push's kernel being
    // enqueued on this same stream BEFORE we enqueue the read — true
    // only with synchronous inline request delivery (the default). With
    // queued delivery the push launch races us: fall back to a normal
    // pull request, which the seq gate orders.
    if (!inline_deliver_ || LocalQueueReq()) return false;
  }
  hipStream_t stream = OneSidedLane(owner, p);
  XPS_HIP_CHECK(hipSetDevice(device_));
  kern::DenseAssign(dst, src, len, stream);
  g_zero_copy_recv.fetch_add(1, std::memory_order_relaxed);
  int64_t bytes = static_cast<int64_t>(len) + 64;
  // the response is delivered to OURSELVES
  Defer(p, stream, nullptr, {.resend = std::move(resp), .bytes = bytes, .local_po = po_});
  p->rx_bytes.fetch_add(bytes, std::memory_order_relaxed);
  return true;
}

bool GpuPlane::EntryPushPull(Message& msg, Peer* p, int64_t* bytes_out) {
  if (!FusedAssignEnabled()) return false;
  if (!(msg.meta.option & kOptPullAddr) || (msg.meta.option & kOptHostAddr)) return false;
  Postoffice* elpo = nullptr;
  GpuPlane* owner = OneSidedOwner(p, &elpo);
  if (!owner) return false;
  SArray<char> vals = msg.data[1];
  size_t len = vals.size();
  if (len == 0) return false;
  char* entry = ResolvePeer(p, msg.meta.entry_addr, len);
  char* dst = static_cast<char*>(HbmPool::Get()->PtrOf(msg.meta.addr, len));
  if (!entry || !dst || !kern::Disjoint3(entry, dst, vals.data(), len)) return false;
  XPS_STAGE(entry_push_pull);
  // queued behind a busy GPU the key joins the open batch of this peer's
  // lane 0 and shares its launch and event. A same-process peer's write
  // runs on the RECEIVER plane's stream, whose completions this plane's
  // queue does not see: it keeps its own launch.
  std::shared_ptr<CoEvent> cev;
  // off by default for this site: with two processes on one GPU the
  // batches of four streams run side by side and the config turned
  // bimodal (2816-3929 GB/s against the parent's 3078-3242)
  static const bool co_one_sided =
      Environment::Get()->GetInt("XPS_COALESCE_ONE_SIDED", 0) != 0;
  if (!elpo && co_one_sided) cev = CoAppend(p, kern::Seg2{entry, dst, vals.data(), len});
  hipStream_t stream = nullptr;
  if (!cev) {
    stream = OneSidedLane(owner, p);
    XPS_HIP_CHECK(hipSetDevice(device_));
    kern::DenseAssign2(entry, dst, vals.data(), len, stream);
    g_fused_launches.fetch_add(1, std::memory_order_relaxed);
  }
  g_fused_assign.fetch_add(1, std::memory_order_relaxed);
  g_zero_copy_recv.fetch_add(1, std::memory_order_relaxed);
  Message note = InPlaceNote(msg, len);
  std::string payload;
  if (!elpo) SerializeNote(&note, /*may_drop_blobs=*/false, &payload);
  int64_t bytes = 64 + static_cast<int64_t>(len);
  Defer(p, stream, std::move(cev),
        {.payload = std::move(payload), .resend = std::move(note),
         .keepalive = KeepAlive(vals), .bytes = bytes, .local_po = elpo});
  p->tx_bytes.fetch_add(bytes, std::memory_order_relaxed);
  *bytes_out = bytes;
  return true;
}

void GpuPlane::EnqueueLocal(Message msg, int64_t bytes) {
  {
    std::lock_guard<std::mutex> lk(local_mu_);
    local_q_.emplace_back(std::move(msg), bytes);
  }
  local_count_.fetch_add(1, std::memory_order_release);
}

// Same-process fast path (joint mode: worker + co-located server share
// the process). This is the reference's IPCTransport/shared_node_mapping_
// locality taken to its limit: no serialization, no ring hop, no poll
// thread — a direct call, with GPU completion still gated by the lane
// event for responses (the requester's buffers must not be released
// before the kernels that read/write them finish).
hipStream_t GpuPlane::ResponseLane(const Message& msg, int peer_id) {
  return (msg.meta.option & kOptPullLane) ? PullStreamForPeer(peer_id) : StreamForPeer(peer_id);
}

void GpuPlane::DrainLanes(int peer_id) {
  for (int l = 0; l < lanes_; ++l) (void)hipStreamSynchronize(StreamLane(peer_id, l));
}

bool GpuPlane::DefersResponse(const Message& msg) const {
  return !msg.meta.request && device_ >= 0 && !KernelLessAck(msg);
}

bool GpuPlane::CopyToHostDest(Peer* p, uint64_t addr, const SArray<char>& vals) {
  void* base = HostShmPool::MapPeer(p->node.host_pool_uid, p->node.host_pool_capacity);
  if (!base || addr > p->node.host_pool_capacity ||
      vals.size() > p->node.host_pool_capacity - addr) {
    return false;
  }
  HostPar::CopyBytes(static_cast<char*>(base) + addr, vals.data(), vals.size());
  return true;
}

hipStream_t GpuPlane::WriteHbmDest(Peer* p, const Message& msg, const SArray<char>& vals) {
  char* dst = ResolvePeer(p, msg.meta.addr, vals.size());
  if (!dst) {
    DrainLanes(p->node.id);
    return nullptr;
  }
  hipStream_t stream = ResponseLane(msg, p->node.id);
  XPS_HIP_CHECK(hipSetDevice(device_));
  // copy KERNEL instead of hipMemcpyAsync: measured 5.2 vs 4.85 TB/s
  // same-device, and it reads/writes hipIpc-mapped peer memory alike
  kern::DenseAssign(dst, vals.data(), vals.size(), stream);
  return stream;
}

void GpuPlane::SerializeNote(Message* note, bool may_drop_blobs, std::string* payload) {
  std::vector<char> all_inline(note->data.size(), 0);
  if (Serialize(*note, all_inline, payload)) return;
  XPS_CHECK(may_drop_blobs) << "in-place note does not fit the ring";
  note->data.clear();
  note->meta.data_type.clear();
  XPS_CHECK(Serialize(*note, {}, payload));
}

void GpuPlane::Defer(Peer* p, hipStream_t stream, std::shared_ptr<CoEvent> cev, Pending pd) {
  XPS_STAGE(defer_queue);
  XPS_CHECK_GE(device_, 0) << "deferred sends are a GPU-plane feature";
  if (!cev) {
    XPS_HIP_CHECK(hipSetDevice(device_));
    pd.ev = GetEvent();
    XPS_HIP_CHECK(hipEventRecord(pd.ev, stream));
  }
  int peer_id = p->node.id;
  pd.peer_id = peer_id;
  pd.cev = std::move(cev);
  {
    std::lock_guard<std::mutex> lk(pend_mu_);
    pending_[peer_id].push_back(std::move(pd));
  }
  pending_count_.fetch_add(1);
  XPS_VLOG(3) << "deferred send queued -> " << peer_id;
}

// Same-process fast path (joint mode: worker + co-located server share
// the process). This is the reference's IPCTransport/shared_node_mapping_
// locality taken to its limit: no serialization, no ring hop, no poll
// thread — a direct call, with GPU completion still gated by the lane
// event for responses (the requester's buffers must not be released
// before the kernels that read/write them finish).
int64_t GpuPlane::SendLocal(Message& msg, Peer* p, Postoffice* lpo) {
  XPS_STAGE(plane_send_local);
  int64_t bytes = 64;
  for (auto& d : msg.data) bytes += static_cast<int64_t>(d.size());

  if (HasPullDest(msg)) {
    SArray<char> vals = msg.data[1];
    // host destination: copy into the requester's buffer NOW, note after
    // (a destination that cannot be mapped takes the plain path below)
    if (HostDest(msg) && CopyToHostDest(p, msg.meta.addr, vals)) {
      g_zero_copy_recv.fetch_add(1, std::memory_order_relaxed);
      Message note = InPlaceNote(msg, vals.size(), NoteBlobs::kSnapshot);
      DeliverLocal(lpo, note, bytes);
      p->tx_bytes.fetch_add(bytes, std::memory_order_relaxed);
      return bytes;
    }
    // HBM destination: run the in-place write now, deliver the note once
    // the copy completes
    if (HbmDest(msg)) {
      hipStream_t stream = WriteHbmDest(p, msg, vals);
      if (!stream) return -1;  // TCP fallback (streams drained first)
      g_zero_copy_recv.fetch_add(1, std::memory_order_relaxed);
      Message note = InPlaceNote(msg, vals.size());
      msg.data.clear();
      Defer(p, stream, nullptr,
            {.resend = std::move(note), .keepalive = KeepAlive(vals), .bytes = bytes,
             .local_po = lpo});
      p->tx_bytes.fetch_add(bytes, std::memory_order_relaxed);
      return bytes;
    }
  }

  if (DefersResponse(msg)) {
    // GPU handler output: deliver once this peer's lane drained
    XPS_STAGE(local_defer);
    // the handler's coalesced dual write: no event of its own, the entry
    // waits for the shared event of its batch
    std::shared_ptr<CoEvent> cev = TakeTicket(p->node.id);
    hipStream_t stream = cev ? nullptr : ResponseLane(msg, p->node.id);
    Defer(p, stream, std::move(cev), {.resend = msg, .bytes = bytes, .local_po = lpo});
  } else {
    // requests, kernel-less acks and every send of a host-only plane go
    // out now. Requests need no copy: the sender's buffers are pinned
    // until the response arrives.
    Message copy = msg;
    if (!msg.meta.request) {
      for (auto& d : copy.data) {
        if (!d.on_device() && d.size()) d = Snapshot(d);
      }
    }
    DeliverLocal(lpo, copy, bytes);
  }
  p->tx_bytes.fetch_add(bytes, std::memory_order_relaxed);
  return bytes;
}

int64_t GpuPlane::Send(Message& msg, const Node& peer_node) {
  XPS_STAGE(plane_send);
  XPS_VLOG(3) << "plane send -> " << peer_node.id << ": " << msg.DebugString();
  Peer* p = GetPeer(peer_node.id);
  {
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->node.shm_uid == 0) p->node = peer_node;
  }

  // ---- one-sided assign push (reference rdma steady state: unsignaled
  // RDMA_WRITE of vals + write-with-imm of meta, rdma_transport.h:341-
  // 356): the worker writes the server's advertised store entry with
  // ITS OWN kernel and sends the meta-only notification once the write
  // completes. The server's push handling shrinks to an ack.
  if (msg.meta.request && msg.meta.push && !msg.meta.pull &&
      (msg.meta.option & kOptEntryPush) && device_ >= 0 && msg.data.size() > 1 &&
      msg.data[1].on_device()) {
    Postoffice* elpo = nullptr;
    GpuPlane* owner = OneSidedOwner(p, &elpo);
    SArray<char> vals = msg.data[1];
    char* dst = owner ? ResolvePeer(p, msg.meta.addr, vals.size()) : nullptr;
    if (dst) {
      XPS_STAGE(entry_push);
      hipStream_t stream = OneSidedLane(owner, p);
      XPS_HIP_CHECK(hipSetDevice(device_));
      kern::DenseAssign(dst, vals.data(), vals.size(), stream);
      g_zero_copy_recv.fetch_add(1, std::memory_order_relaxed);
      Message note = InPlaceNote(msg, vals.size());
      std::string payload;
      if (!elpo) SerializeNote(&note, /*may_drop_blobs=*/false, &payload);
      int64_t bytes = 64 + static_cast<int64_t>(vals.size());
      Defer(p, stream, nullptr,
            {.payload = std::move(payload), .resend = std::move(note),
             .keepalive = KeepAlive(vals), .bytes = bytes, .local_po = elpo});
      p->tx_bytes.fetch_add(bytes, std::memory_order_relaxed);
      return bytes;
    }
    msg.meta.option &= ~kOptEntryPush;  // entry unmapped: normal path
  }

  // ---- one-sided FUSED push+pull: same idea, one dual-write kernel.
  // kOptInPlace on the caller's msg reports that the write really ran
  // (KVWorker::Send keeps its one_sided flag honest from it).
  if (msg.meta.request && msg.meta.push && msg.meta.pull && (msg.meta.option & kOptEntryPush)) {
    int64_t bytes = 0;
    if (device_ >= 0 && msg.data.size() > 1 && msg.data[1].on_device() &&
        EntryPushPull(msg, p, &bytes)) {
      msg.meta.option |= kOptInPlace;
      return bytes;
    }
    msg.meta.option &= ~kOptEntryPush;  // declined: normal fused request
    msg.meta.entry_addr = 0;
  }

  if (Postoffice* lpo = LocalPeer(p)) return SendLocal(msg, p, lpo);
  bool response = !msg.meta.request;
  if (!EnsureRing(p)) {
    if (response && device_ >= 0) DrainLanes(peer_node.id);
    return -1;
  }

  if (HasPullDest(msg)) {
    SArray<char> vals = msg.data[1];
    // host destination: memcpy now, then the note over the ring
    if (HostDest(msg)) {
      if (!CopyToHostDest(p, msg.meta.addr, vals)) return -1;  // unmappable: TCP fallback
      Message note = InPlaceNote(msg, vals.size(), NoteBlobs::kInlineOnly);
      std::string payload;
      SerializeNote(&note, /*may_drop_blobs=*/true, &payload);
      int64_t bytes = static_cast<int64_t>(vals.size() + payload.size());
      auto ring = RingOf(p);
      if (!ring || !ring->Push(payload.data(), static_cast<uint32_t>(payload.size()))) return -1;
      p->tx_bytes.fetch_add(bytes, std::memory_order_relaxed);
      return bytes;
    }
    // HBM destination: one-sided xGMI write, the note follows its event
    if (HbmDest(msg)) {
      hipStream_t stream = WriteHbmDest(p, msg, vals);
      if (!stream) return -1;  // TCP fallback (streams drained first)
      Message note = InPlaceNote(msg, vals.size());
      std::string payload;
      SerializeNote(&note, /*may_drop_blobs=*/true, &payload);
      int64_t bytes = static_cast<int64_t>(vals.size() + payload.size());
      msg.data.clear();
      // The note is also the TCP-resendable form: by the time a fallback
      // happens the event has fired, i.e. the in-place write already
      // landed in the peer's pool.
      Defer(p, stream, nullptr,
            {.payload = std::move(payload), .resend = std::move(note),
             .keepalive = KeepAlive(vals), .bytes = bytes});
      p->tx_bytes.fetch_add(bytes, std::memory_order_relaxed);
      return bytes;
    }
  }

  // ---- general path: inline blobs + by-ref device/host-pool blobs ----
  std::vector<char> by_ref(msg.data.size(), 0);
  int64_t ref_bytes = 0;
  for (size_t i = 0; i < msg.data.size(); ++i) {
    if (msg.data[i].on_device()) {
      by_ref[i] = 1;
      ref_bytes += msg.data[i].size();
      if (i == 1) msg.meta.option |= kOptValsByRef;
    } else if (msg.data[i].size() > kInlineMax) {
      by_ref[i] = 2;  // CanSend verified host-pool membership
      ref_bytes += msg.data[i].size();
    }
  }
  std::string payload;
  if (!Serialize(msg, by_ref, &payload)) {
    if (response && device_ >= 0) (void)hipStreamSynchronize(StreamForPeer(peer_node.id));
    return -1;
  }
  int64_t bytes = static_cast<int64_t>(payload.size()) + ref_bytes;
  if (DefersResponse(msg)) {
    // order behind any handler kernels on this peer's lane. The resend
    // copy doubles as the keepalive (shallow: SArrays shared).
    Defer(p, ResponseLane(msg, peer_node.id), nullptr,
          {.payload = std::move(payload), .resend = msg, .bytes = bytes});
  } else {
    // requests, kernel-less acks and every send of a host-only plane go
    // out now (host responses were produced synchronously; nothing to
    // wait for)
    auto ring = RingOf(p);
    if (!ring || !ring->Push(payload.data(), static_cast<uint32_t>(payload.size()))) return -1;
    XPS_VLOG(3) << "plane send done -> " << peer_node.id;
  }
  p->tx_bytes.fetch_add(bytes, std::memory_order_relaxed);
  return bytes;
}

void GpuPlane::CompletionLoop() {
  XPS_HIP_CHECK(hipSetDevice(device_));
  // 1 µs timer slack: the default 50 µs slack turns the idle usleep into
  // a ~70 µs latency floor per hop (dominates small-message RTT)
  prctl(PR_SET_TIMERSLACK, 1000);
  const int kSpin = Environment::Get()->GetInt("XPS_POLL_SPIN", 200000);
  int idle = 0;
  // NOTE on locking: pend_mu_ is held only for deque push/pop/front
  // snapshots, never across hipEventQuery or ring pushes — holding it
  // through the poll loop put ~6 µs of lock contention into EVERY
  // deferred response (measured via XPS_TIMING, round 2). This thread is
  // the only popper, so a front observed ready stays front until we pop.
  std::vector<int> ids;
  while (!stop_.load()) {
    bool did = false;
    if (pending_count_.load(std::memory_order_acquire) > 0) {
      ids.clear();
      {
        std::lock_guard<std::mutex> lk(pend_mu_);
        for (auto& kv : pending_) {
          if (!kv.second.empty()) ids.push_back(kv.first);
        }
      }
      for (int id : ids) {
        while (!stop_.load()) {
          hipEvent_t front_ev = nullptr;
          std::shared_ptr<CoEvent> cev;
          {
            std::lock_guard<std::mutex> lk(pend_mu_);
            auto& dq = pending_[id];
            if (dq.empty()) break;
            front_ev = dq.front().ev;
            cev = dq.front().cev;
          }
          bool retired = false;
          if (cev) {
            // entry of a coalesced launch: not ready before its batch is
            // launched (this thread launches a batch that reached the
            // front); one successful query then releases every
            // consecutive entry of the batch
            front_ev = cev->ev.load(std::memory_order_acquire);
            if (!front_ev) {
              if (!CoFrontUnlaunched(GetPeer(id), cev)) break;
              continue;
            }
          }
          if (!cev || !cev->done.load(std::memory_order_acquire)) {
            hipError_t e = hipEventQuery(front_ev);
            if (e == hipErrorNotReady) break;
            XPS_CHECK(e == hipSuccess) << "hipEventQuery: " << hipGetErrorString(e);
            if (cev) {
              cev->done.store(true, std::memory_order_release);
              retired = true;
            }
          }
          XPS_STAGE(defer_release);
          if (retired) CoRetired(GetPeer(id));
          Pending front;
          {
            std::lock_guard<std::mutex> lk(pend_mu_);
            auto& dq = pending_[id];
            front = std::move(dq.front());
            dq.pop_front();
          }
          pending_count_.fetch_sub(1);
          if (front.local_po) {  // same-process: direct delivery
            DeliverLocal(front.local_po, front.resend, front.bytes);
            if (front.ev) PutEvent(front.ev);  // a coalesced entry's event is shared
            did = true;
            continue;
          }
          Peer* peer = GetPeer(front.peer_id);
          auto ring = peer ? RingOf(peer) : nullptr;
          bool sent = ring && ring->Push(front.payload.data(),
                                         static_cast<uint32_t>(front.payload.size()));
          if (sent) {
            XPS_VLOG(3) << "deferred send done -> " << front.peer_id;
          } else {
            // never drop: the requester is blocked in Wait on this
            // response — deliver it over the TCP path instead
            XPS_LOG(Warning) << "deferred plane send failed -> " << front.peer_id
                             << "; falling back to TCP";
            if (po_->van()->SendOverTcp(front.resend, front.peer_id) < 0) {
              XPS_LOG(Warning) << "TCP fallback to " << front.peer_id
                               << " failed too (peer dead?)";
            }
          }
          if (front.ev) PutEvent(front.ev);  // a coalesced entry's event is shared
          did = true;
        }
      }
    }
    if (did) {
      idle = 0;
    } else if (++idle > kSpin) {
      usleep(20);
    }
  }
}

void GpuPlane::RingPollLoop() {
  if (device_ >= 0) XPS_HIP_CHECK(hipSetDevice(device_));
  prctl(PR_SET_TIMERSLACK, 1000);
  const int kSpin = Environment::Get()->GetInt("XPS_POLL_SPIN", 200000);
  std::vector<char> buf(ShmRing::MaxPayload());
  int idle = 0;
  std::deque<std::pair<Message, int64_t>> local;
  while (!stop_.load()) {
    // same-process deliveries first (they need no parsing)
    if (local_count_.load(std::memory_order_acquire) > 0) {
      {
        std::lock_guard<std::mutex> lk(local_mu_);
        local.swap(local_q_);
      }
      local_count_.fetch_sub(static_cast<int>(local.size()));
      for (auto& lm : local) {
        XPS_STAGE(local_handle);
        HandToVan(po_->van(), lm.first, lm.second, true);
      }
      idle = 0;
      local.clear();
    }
    uint32_t n = in_ring_.Pop(buf.data());
    if (n == 0) {
      if (++idle > kSpin) usleep(20);
      continue;
    }
    idle = 0;
    XPS_STAGE(ring_handle);
    ByteReader r(buf.data(), n);
    uint64_t meta_len = r.U64();
    Message msg;
    {
      std::vector<char> meta(meta_len);
      r.Raw(meta.data(), meta_len);
      UnpackMeta(meta.data(), meta_len, &msg.meta);
    }
    int nblobs = r.U8();
    int64_t ref_bytes = 0;
    bool ok = true;
    for (int i = 0; i < nblobs; ++i) {
      int kind = r.U8();
      if (kind == 0) {
        uint64_t len = r.U64();
        SArray<char> d(len);
        r.Raw(d.data(), len);
        msg.data.push_back(d);
      } else if (kind == 1) {
        uint64_t off = r.U64();
        uint64_t len = r.U64();
        Peer* sender = GetPeer(msg.meta.sender);
        char* ptr = sender ? ResolvePeer(sender, off, len) : nullptr;
        if (!ptr) {
          XPS_LOG(Warning) << "dropping by-ref blob: sender pool not mapped (from "
                           << msg.meta.sender << ")";
          ok = false;
          break;
        }
        msg.data.push_back(SArray<char>(ptr, len, device_));
        ref_bytes += len;
        g_zero_copy_recv.fetch_add(1, std::memory_order_relaxed);
      } else {  // kind 2: host shm pool
        uint64_t off = r.U64();
        uint64_t len = r.U64();
        Peer* sender = GetPeer(msg.meta.sender);
        void* base = sender ? HostShmPool::MapPeer(sender->node.host_pool_uid,
                                                   sender->node.host_pool_capacity)
                            : nullptr;
        if (!base || off > sender->node.host_pool_capacity ||
            len > sender->node.host_pool_capacity - off) {
          XPS_LOG(Warning) << "dropping host-ref blob: sender host pool not mapped (from "
                           << msg.meta.sender << ")";
          ok = false;
          break;
        }
        msg.data.push_back(SArray<char>(static_cast<char*>(base) + off, len, kCPU));
        ref_bytes += len;
        g_zero_copy_recv.fetch_add(1, std::memory_order_relaxed);
      }
    }
    if (!ok) continue;
    XPS_VLOG(3) << "ring recv: " << msg.DebugString();
    if (msg.meta.sender != kEmptyNodeID) {
      GetPeer(msg.meta.sender)->rx_bytes.fetch_add(n + ref_bytes, std::memory_order_relaxed);
    }
    // by-reference blobs were counted above, while they were resolved
    HandToVan(po_->van(), msg, n + ref_bytes, false);
  }
}

std::shared_ptr<DataPlane> CreateGpuPlane(Postoffice* po, int device) {
  // device < 0 builds the host-only variant (shm rings + host pool)
  return std::make_shared<GpuPlane>(po, device);
}

}  // namespace xps
