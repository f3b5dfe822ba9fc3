"""Run enumeration of the batched dual-write kernel (csrc/tile_runs.h):
which pieces of which segments one block's tile covers. The kernel runs
the same function on the scalar side; here it runs on the host, no GPU."""
import random

import pytest

import ps_lite_amd as ps

_runs = ps._core.tile_runs


def _cases():
    out = []
    for seed in range(300):
        rng = random.Random(seed)
        nseg = rng.randint(1, 64)
        if seed % 3 == 0:
            counts = [rng.randint(1, 5000) for _ in range(nseg)]
        elif seed % 3 == 1:  # many tiny segments per tile
            counts = [rng.randint(1, 40) for _ in range(nseg)]
        else:  # sizes at and next to tile multiples
            counts = [rng.choice([1, 255, 256, 257, 511, 512, 513, 768, 5000])
                      for _ in range(nseg)]
        tile = 256 * rng.randint(1, 24)
        out.append((seed, counts, tile))
    return out


_CASES = _cases()


def _check(counts, tile):
    total = sum(counts)
    nblocks = (total + tile - 1) // tile
    flat = []  # (global chunk begin, global chunk end) of every run, in block order
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + c)
    for b in range(nblocks):
        runs = _runs(counts, tile, b)
        assert runs, (b, "a block inside the grid has work")
        prev_seg = -1
        at = b * tile
        for seg, lo, hi in runs:
            assert 0 <= seg < len(counts)
            assert lo < hi <= counts[seg], "no run is empty or leaves its segment"
            assert seg > prev_seg, "runs are in segment order, one per segment"
            assert offs[seg] + lo == at, "runs follow each other without a gap"
            at = offs[seg] + hi
            prev_seg = seg
            flat.append((offs[seg] + lo, offs[seg] + hi))
        # a tile ends at its boundary, the last one at the total
        assert at == min((b + 1) * tile, total)
    # every chunk of every segment exactly once: the runs tile [0, total)
    at = 0
    for lo, hi in flat:
        assert lo == at
        at = hi
    assert at == total
    # past the grid: nothing
    assert _runs(counts, tile, nblocks) == []
    assert _runs(counts, tile, nblocks + 7) == []


@pytest.mark.parametrize("lo", range(0, len(_CASES), 50))
def test_runs_cover_every_chunk_once(lo):
    for seed, counts, tile in _CASES[lo:lo + 50]:
        _check(counts, tile)


def test_single_chunk_and_exact_fit():
    assert _runs([1], 256, 0) == [(0, 0, 1)]
    assert _runs([256, 256], 256, 0) == [(0, 0, 256)]
    assert _runs([256, 256], 256, 1) == [(1, 0, 256)]
    assert _runs([257, 255, 1, 513], 512, 0) == [(0, 0, 257), (1, 0, 255)]
    assert _runs([257, 255, 1, 513], 512, 1) == [(2, 0, 1), (3, 0, 511)]
    assert _runs([257, 255, 1, 513], 512, 2) == [(3, 511, 513)]


def test_rejects_empty_segment_and_tile():
    with pytest.raises(ValueError):
        _runs([4, 0, 4], 256, 0)
    with pytest.raises(ValueError):
        _runs([4], 0, 0)


# The launchers' tile rule (TileChunks in csrc/tile_runs.h) against the three
# formulas it replaced, written out: (stride, want_blocks, max_tile) per policy.
_ANY = 2**64 - 1
_POLICIES = {
    "balanced": (256, 8192, 0),
    "dual_write": (256, 8192, 512),
    "mxfp8": (8, _ANY, 0),
}
_TOTALS = [1, 255, 256, 257, 8192 * 256 - 1, 8192 * 256, 8192 * 256 + 1, 8192 * 512 + 1,
           2**32 + 5]
_CAPS = [0, 1, 2, 3, 5, 8192, 10000]


def _ceil(a, b):
    return (a + b - 1) // b


def _old_tile(policy, total, cap):
    if policy == "mxfp8":
        spb = 8
        if cap > 0:
            spb = _ceil(_ceil(total, cap), 8) * 8
        return spb
    max_blocks = min(cap, 8192) if cap > 0 else 8192
    cpb = _ceil(_ceil(total, max_blocks), 256) * 256
    if policy == "dual_write" and cap <= 0 and cpb > 512:
        cpb = 512
    return cpb


@pytest.mark.parametrize("policy", sorted(_POLICIES))
def test_tile_size_matches_the_three_policies(policy):
    stride, want, max_tile = _POLICIES[policy]
    for total in _TOTALS:
        for cap in _CAPS:
            tile = ps._core.tile_size(total, stride, want, max_tile, cap)
            assert tile == _old_tile(policy, total, cap), (total, cap)
            assert tile > 0 and tile % stride == 0, (total, cap)
            blocks = _ceil(total, tile)
            assert blocks * tile >= total > (blocks - 1) * tile, (total, cap)
            if cap > 0:
                assert blocks <= cap, (total, cap)


def test_tile_size_rejects_zero():
    for args in [(0, 256, 8192, 0, 0), (1, 0, 8192, 0, 0), (1, 256, 0, 0, 0)]:
        with pytest.raises(ValueError):
            ps._core.tile_size(*args)
