// Admit-or-flush decision of the dual-write launch coalescer
// (gpu_plane.cc): may a new {dst0, dst1, src, nbytes} segment join the
// open batch of its stream? Pure host code, no HIP — testable without a
// GPU (tests/test_coalesce_admit.py).
#pragma once

#include <cstddef>
#include <cstdint>

namespace xps {
namespace kern {

// one fused push+pull inside a batched dual-write launch:
// dst0[i] = dst1[i] = src[i] over nbytes
struct Seg2 {
  void* dst0;
  void* dst1;
  const void* src;
  size_t nbytes;
};

static const int kMaxBatch2 = 64;  // == kern::kMaxBatch (kernels.h asserts it)

enum class Admit {
  kAdmit,       // append to the open batch
  kFlushFirst,  // launch the open batch, then append to a fresh one
  kReject,      // never batched: the caller flushes and launches directly
};

inline bool RangesOverlap(const void* a, const void* b, size_t alen, size_t blen) {
  uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
  return p < q + blen && q < p + alen;
}

// Within one launch segments run concurrently, so the batch must be free
// of write-write and read-write hazards: the newcomer's destinations may
// touch no range of an earlier segment, and its source no earlier
// destination (source/source sharing is harmless). A hazard — typically
// the same key twice in one burst — flushes first, which restores stream
// order between the two. Rejected outright: an empty, misaligned or
// non-16 B-multiple segment (the batched kernel moves 16 B chunks only),
// one whose own three ranges overlap, and a segment offered to a batch
// that is already full.
inline Admit CoalesceAdmit(const Seg2* open, int n_open, const Seg2& s) {
  uintptr_t bits = reinterpret_cast<uintptr_t>(s.dst0) | reinterpret_cast<uintptr_t>(s.dst1) |
                   reinterpret_cast<uintptr_t>(s.src) | static_cast<uintptr_t>(s.nbytes);
  if (s.nbytes == 0 || (bits & 15u) != 0) return Admit::kReject;
  if (RangesOverlap(s.dst0, s.dst1, s.nbytes, s.nbytes) ||
      RangesOverlap(s.dst0, s.src, s.nbytes, s.nbytes) ||
      RangesOverlap(s.dst1, s.src, s.nbytes, s.nbytes)) {
    return Admit::kReject;
  }
  if (n_open >= kMaxBatch2) return Admit::kReject;
  for (int i = 0; i < n_open; ++i) {
    const Seg2& o = open[i];
    const void* theirs[3] = {o.dst0, o.dst1, o.src};
    for (const void* t : theirs) {
      if (RangesOverlap(s.dst0, t, s.nbytes, o.nbytes) ||
          RangesOverlap(s.dst1, t, s.nbytes, o.nbytes)) {
        return Admit::kFlushFirst;
      }
    }
    if (RangesOverlap(s.src, o.dst0, s.nbytes, o.nbytes) ||
        RangesOverlap(s.src, o.dst1, s.nbytes, o.nbytes)) {
      return Admit::kFlushFirst;
    }
  }
  return Admit::kAdmit;
}

}  // namespace kern
}  // namespace xps
