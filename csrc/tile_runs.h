// Tiling of the batched kernels' concatenated unit space (kernels.hip,
// mxfp8.hip). Run enumeration: which pieces of which segments does one
// block's tile cover? Pure arithmetic on block-uniform values, no HIP
// calls — the kernels run it on the scalar side, the host runs the very
// same code in tests/test_tile_runs.py (no GPU needed). And the launchers'
// tile rule, tested there too.
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

// Tile size of a batched launch over `total` units: enough tiles for
// want_blocks blocks (fewer under a tile_cap > 0, the tests' cap on the
// grid), in whole multiples of `stride`, the units one sweep of the block
// covers. max_tile > 0 bounds the tile, so that a large launch grows its
// grid instead; a tile_cap is obeyed as given and lifts that bound.
constexpr unsigned long long kAnyBlocks = ~0ull;  // want_blocks: one stride per tile
inline unsigned long long TileChunks(unsigned long long total, unsigned long long stride,
                                     unsigned long long want_blocks,
                                     unsigned long long max_tile, int tile_cap) {
  unsigned long long blocks = want_blocks;
  if (tile_cap > 0 && static_cast<unsigned long long>(tile_cap) < blocks) blocks = tile_cap;
  unsigned long long tile = total / blocks + (total % blocks != 0);
  tile = (tile + stride - 1) / stride * stride;
  if (tile_cap <= 0 && max_tile > 0 && tile > max_tile) tile = max_tile;
  return tile;
}

// blocks that cover `total` units in tiles of `tile`
inline unsigned TileGrid(unsigned long long total, unsigned long long tile) {
  return static_cast<unsigned>((total + tile - 1) / tile);
}

}  // namespace kern
}  // namespace xps
