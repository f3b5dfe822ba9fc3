"""Shapes at which the dual-write kernels' structure can go wrong: the
batched kernel takes each block's tile apart into per-segment runs
(csrc/tile_runs.h) and sweeps every run with the whole block, the per-key
kernel sweeps a grid stride and a byte tail. Byte-exact against both
destinations, the guard bytes around them and the untouched source.
All marked gpu; everything stays under a few MiB."""
import pytest

import ps_lite_amd as ps

pytestmark = pytest.mark.gpu

_GUARD = 0xAB
_LEAD, _TRAIL = 16, 48  # guard bytes around every destination range
_REM = [0, 1, 255, 256, 257]

_BOUNDARY = [16 * 257, 16 * 255, 16, 16 * 513]  # boundaries mid-wave and mid-block
_BATCHED_CASES = (
    [("boundary_cap%d" % c, _BOUNDARY, c) for c in (1, 2, 3, 0)] +
    [("many16", [16] * 64, 0)] +
    [("rem%d" % r, [16 * (2048 + r)], 0) for r in _REM] +
    [("rem%d_then48" % r, [16 * (2048 + r), 48], 0) for r in _REM] +
    # totals that are no multiple of the tile: the last tile is short
    [("short_last", [16 * (512 * 3 + 77)], 0),
     ("short_last_cap2", [16 * (512 * 3 + 77), 16 * 3], 2),
     ("short_last_cap5", [16 * 1000, 16 * 1000, 16 * 1001], 5)]
)


def _torch():
    import torch
    return torch


@pytest.mark.parametrize("name,sizes,tile_cap", _BATCHED_CASES,
                         ids=[c[0] for c in _BATCHED_CASES])
def test_batched_assign2_shapes(name, sizes, tile_cap):
    torch = _torch()
    g = torch.Generator(device="cpu").manual_seed(sum(sizes) * 7 + len(sizes) * 131 + tile_cap)
    total = sum(sizes)
    src = torch.randint(0, 256, (total,), dtype=torch.uint8, generator=g)
    src_d = src.to("cuda:0")
    span = sum(s + _LEAD + _TRAIL for s in sizes)
    expect = torch.full((span,), _GUARD, dtype=torch.uint8)
    bufs = [torch.full((span,), _GUARD, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    segs, s_at, d_at = [], 0, 0
    for n in sizes:
        d_at += _LEAD
        segs.append((bufs[0].data_ptr() + d_at, bufs[1].data_ptr() + d_at,
                     src_d.data_ptr() + s_at, n))
        expect[d_at:d_at + n] = src[s_at:s_at + n]
        d_at += n + _TRAIL
        s_at += n
    ps._core.k_batched_assign2(segs, tile_cap)
    for b in bufs:  # payload and every guard byte at once
        assert torch.equal(b.cpu(), expect)
    assert torch.equal(src_d.cpu(), src)


def _dense(nbytes, grid_cap, lead):
    """Destinations start `lead` bytes into guard-filled buffers, the source
    `lead % 16` bytes into its own (so a misaligned lead misaligns all three)."""
    torch = _torch()
    g = torch.Generator(device="cpu").manual_seed(nbytes * 3 + grid_cap)
    skew = lead % 16
    src = torch.randint(0, 256, (skew + nbytes + 16,), dtype=torch.uint8, generator=g)
    src_d = src.to("cuda:0")
    expect = torch.full((lead + nbytes + _TRAIL,), _GUARD, dtype=torch.uint8)
    expect[lead:lead + nbytes] = src[skew:skew + nbytes]
    bufs = [torch.full((lead + nbytes + _TRAIL,), _GUARD, dtype=torch.uint8, device="cuda:0")
            for _ in range(2)]
    ps._core.k_dense_assign2(bufs[0].data_ptr() + lead, bufs[1].data_ptr() + lead,
                             src_d.data_ptr() + skew, nbytes, grid_cap)
    for b in bufs:
        assert torch.equal(b.cpu(), expect)
    assert torch.equal(src_d.cpu(), src)


# every remainder meets a different tail length in 1..15
_DENSE_CASES = [(16 * (2048 + r) + tail, cap)
                for (r, tail) in zip(_REM, [1, 15, 7, 8, 3]) for cap in (1, 2)]


@pytest.mark.parametrize("nbytes,grid_cap", _DENSE_CASES)
def test_dense_assign2_capped_grid_with_tail(nbytes, grid_cap):
    _dense(nbytes, grid_cap, lead=16)


@pytest.mark.parametrize("grid_cap", [0, 1, 2])
def test_dense_assign2_misaligned_takes_byte_loop(grid_cap):
    _dense(16 * 300 + 5, grid_cap, lead=4)
