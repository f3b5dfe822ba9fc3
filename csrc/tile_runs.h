// Run enumeration of the batched dual-write kernel (kernels.hip): which
// pieces of which segments does one block's tile of the concatenated
// 16 B-chunk space cover? Pure arithmetic on block-uniform values, no
// HIP calls — the kernel runs it on the scalar side, the host runs the
// very same code in tests/test_tile_runs.py (no GPU needed).
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define XPS_HOST_DEVICE __host__ __device__
#else
#define XPS_HOST_DEVICE
#endif

namespace xps {
namespace kern {

// chunks [lo, hi) of segment seg, counted from the segment's own start;
// never empty
struct TileRun {
  int seg;
  unsigned long long lo, hi;
};

// position in the concatenated space: the next run starts at chunk pos
// (inside segment seg) and the range ends at chunk end
struct TileRunIter {
  int seg;
  unsigned long long pos, end;
};

// Iterator over chunks [begin, end) of the concatenated space. prefix
// holds the n segments' exclusive chunk offsets, prefix[n] = total, and is
// strictly increasing (no empty segment). end is clamped to the total; an
// empty or out-of-range request yields no run.
XPS_HOST_DEVICE inline TileRunIter TileRunsRange(const unsigned long long* prefix, int n,
                                                 unsigned long long begin,
                                                 unsigned long long end) {
  TileRunIter it;
  unsigned long long total = prefix[n];
  it.end = end < total ? end : total;
  it.pos = begin;
  it.seg = 0;
  if (it.pos >= it.end) {
    it.pos = it.end;
    return it;
  }
  // last segment whose offset is <= begin
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= begin) {
      lo = mid;
    } else {
      hi = mid - 1;
    }
  }
  it.seg = lo;
  return it;
}

// the tile of block block_index when every block owns chunks_per_block
// consecutive chunks
XPS_HOST_DEVICE inline TileRunIter TileRunsBegin(const unsigned long long* prefix, int n,
                                                 unsigned long long chunks_per_block,
                                                 unsigned long long block_index) {
  unsigned long long begin = block_index * chunks_per_block;
  return TileRunsRange(prefix, n, begin, begin + chunks_per_block);
}

// Next run, in order; false once the range is used up.
XPS_HOST_DEVICE inline bool TileRunsNext(const unsigned long long* prefix, TileRunIter* it,
                                         TileRun* run) {
  if (it->pos >= it->end) return false;
  unsigned long long seg_lo = prefix[it->seg], seg_hi = prefix[it->seg + 1];
  unsigned long long stop = seg_hi < it->end ? seg_hi : it->end;
  run->seg = it->seg;
  run->lo = it->pos - seg_lo;
  run->hi = stop - seg_lo;
  it->pos = stop;
  ++it->seg;
  return true;
}

}  // namespace kern
}  // namespace xps
