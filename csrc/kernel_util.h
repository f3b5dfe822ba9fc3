// What the kernel files (kernels.hip, mxfp8.hip) share on the host side:
// block size, grid rule, alignment test, and the segment table of the
// batched kernels with the loop that fills it. kernels.h, the header of the
// public launchers, includes this one for Aligned16 and kMaxBatch, so every
// includer of kernels.h sees these names in xps::kern; only the two kernel
// files are meant to use the rest.
#pragma once

#include <cstddef>
#include <cstdint>

namespace xps {
namespace kern {

constexpr int kBlock = 256;

// blocks of kBlock for `units` work items: at most block_cap, at most
// grid_cap where that is > 0 (the tests' grid_cap / tile_cap arguments),
// never zero
inline int GridFor(size_t units, int block_cap, int grid_cap) {
  size_t g = (units + kBlock - 1) / kBlock;
  if (g > static_cast<size_t>(block_cap)) g = block_cap;
  if (grid_cap > 0 && g > static_cast<size_t>(grid_cap)) g = grid_cap;
  return static_cast<int>(g ? g : 1);
}

// the 16 B forms of the kernels need every pointer they touch 16 B-aligned
// (pool buffers are); anything else takes the element form
template <class... Ptrs>
inline bool Aligned16(const Ptrs*... p) {
  return ((reinterpret_cast<uintptr_t>(p) | ...) & 15u) == 0;
}

// segments per batched launch
static const int kMaxBatch = 64;

// The batched kernels' argument: up to kMaxBatch segments concatenated
// into one space of units (16 B chunks, or MXFP8 superblocks). prefix
// holds the exclusive unit offsets, prefix[n] = total, strictly
// increasing: no segment of a table is empty.
template <class Seg>
struct SegTable {
  Seg d[kMaxBatch];
  unsigned long long prefix[kMaxBatch + 1];
  int n;
};

// Cuts segs[0, n) into tables of up to kMaxBatch non-empty segments and
// calls launch(table, total units) for each; a segment of units(seg) == 0
// joins no table, and a list without a non-empty segment launches nothing.
// Returns the number of launches.
template <class Seg, class Units, class Launch>
int ForEachTable(const Seg* segs, int n, Units units, Launch launch) {
  int launches = 0;
  int off = 0;
  while (off < n) {
    SegTable<Seg> t{};
    unsigned long long total = 0;
    while (off < n && t.n < kMaxBatch) {
      const Seg& sg = segs[off++];
      unsigned long long u = units(sg);
      if (u == 0) continue;  // keeps prefix strictly increasing
      t.d[t.n] = sg;
      t.prefix[t.n] = total;
      total += u;
      ++t.n;
    }
    t.prefix[t.n] = total;
    if (total == 0) continue;
    launch(t, total);
    ++launches;
  }
  return launches;
}

}  // namespace kern
}  // namespace xps
