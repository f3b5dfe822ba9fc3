"""The MXFP8 wire format on the CPU: the host reference of csrc/mxfp8.h
(software e4m3 round-to-nearest-even) against the torch model of
mxfp8_model.py, and the properties the format promises."""
import threading

import numpy as np
import pytest
import torch

import mxfp8_model as model
import ps_lite_amd as ps
from ps_lite_amd import ops

_core = ps._core
_PORT = [31500]


def _gaussian(n, seed=0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _heavy(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * torch.exp(3 * torch.randn(n, generator=g))


def _edge_blocks():
    """Blocks of zeros, and blocks whose scaled amax is exactly 448, 449,
    464, 465 and 511 (either side of the bump and of the e4m3 rounding
    boundary above 448), at several exponents and both signs."""
    g = torch.Generator().manual_seed(2)
    blocks = [torch.zeros(32), torch.zeros(32)]
    for k in (-40, -5, 0, 7, 60):
        for top in (448.0, 449.0, 464.0, 465.0, 511.0, 256.0, 447.0):
            b = (torch.rand(32, generator=g) * 2 - 1) * 255.0
            b[int(torch.randint(0, 32, (1,), generator=g))] = top if k % 2 else -top
            blocks.append(torch.ldexp(b, torch.tensor(k)))
    blocks.append(torch.zeros(32))
    return torch.cat(blocks)


_INPUTS = {
    "gaussian": _gaussian(65536),
    "heavy": _heavy(65536),
    "edges": _edge_blocks(),
}


def _host_q(x):
    return _core.mxfp8_quantize_host(x.numpy())


def _check_against_model(x):
    n = x.numel()
    packed = _host_q(x)
    assert packed.dtype == np.uint8 and packed.size == model.packed_nbytes(n)
    byte, codes = model.quantize(x)
    model.assert_packed_equal(packed, model.pack(byte, codes))
    want = model.dequantize(byte, codes, n)
    got = torch.from_numpy(_core.mxfp8_dequantize_host(packed, n))
    assert torch.equal(got, want)
    third = torch.from_numpy(_core.mxfp8_dequantize_host(packed, n, alpha=1.0 / 3.0))
    assert torch.equal(third, model.dequantize(byte, codes, n, alpha=1.0 / 3.0))


@pytest.mark.parametrize("name", sorted(_INPUTS))
def test_host_reference_equals_model(name):
    _check_against_model(_INPUTS[name])


def test_edge_blocks_hit_the_bump():
    """The host reference on the edge input, against the scale rule written
    out here: a scaled amax above 448 bumps the scale byte, 448 itself does
    not, and no code saturates past amax. The same asserts confirm that the
    input holds the cases it claims."""
    x = _INPUTS["edges"]
    byte, codes = model.unpack(_host_q(x))
    amax = x.view(-1, 32).abs().amax(dim=1)
    be = ((amax.view(torch.int32) >> 23) & 0xff)
    floor_byte = (be - 8).clamp(min=0)
    scaled = torch.ldexp(amax, 127 - floor_byte)
    assert set(scaled.tolist()) >= {0.0, 448.0, 449.0, 464.0, 465.0, 511.0}
    want = floor_byte + (scaled > 448).to(torch.int32)
    assert torch.equal(byte[:want.numel()].to(torch.int32), want)  # the rest is padding
    assert not byte[want.numel():].any()
    back = torch.from_numpy(_core.mxfp8_dequantize_host(_host_q(x), x.numel()))
    assert torch.equal(back, model.dequantize(byte, codes, x.numel()))
    back = back.view(-1, 32).abs().amax(dim=1)
    assert bool((back >= amax * (1 - 1 / 16)).all())


@pytest.mark.parametrize("n", [1, 31, 32, 33, 511, 512, 513])
def test_host_reference_any_length(n):
    _check_against_model(_gaussian(n, seed=10 + n))
    _check_against_model(_heavy(n, seed=20 + n))
    # elements past n count as +0.0: the padding holds zero codes
    packed = _host_q(_gaussian(n, seed=10 + n))
    byte, codes = model.unpack(packed)
    tail = model.dequantize(byte, codes, byte.numel() * 32)[n:]
    assert not tail.any()


@pytest.mark.parametrize("name", sorted(_INPUTS))
def test_value_idempotence(name):
    x = _INPUTS[name]
    once = model.roundtrip(x)
    assert torch.equal(model.roundtrip(once), once)
    n = x.numel()
    host_once = _core.mxfp8_dequantize_host(_host_q(x), n)
    host_twice = _core.mxfp8_dequantize_host(_core.mxfp8_quantize_host(host_once), n)
    assert np.array_equal(host_twice, host_once)


@pytest.mark.parametrize("name", sorted(_INPUTS))
def test_error_bound_per_block(name):
    """|err| <= block amax / 16. A scaled amax in [256, 448] meets e4m3
    steps of at most 32, so rounding errs by at most 16 <= amax / 16; a
    bumped one in (224, 256) meets steps of at most 16, so by 8 < amax / 16.
    Nothing saturates, since no scaled value exceeds 448."""
    x = _INPUTS[name]
    got = torch.from_numpy(_core.mxfp8_dequantize_host(_host_q(x), x.numel()))
    err = (got - x).abs().view(-1, 32).amax(dim=1)
    amax = x.view(-1, 32).abs().amax(dim=1)
    assert bool((err <= amax / 16).all()), float((err / amax.clamp(min=1e-38)).max())


def test_packed_nbytes():
    for n, want in [(0, 0), (1, 528), (32, 528), (512, 528), (513, 1056), (1024, 1056),
                    (70001, 137 * 528), (1 << 24, (1 << 15) * 528)]:
        assert ops.mxfp8_packed_nbytes(n) == want
        assert _core.mxfp8_packed_nbytes(n) == want
        assert model.packed_nbytes(n) == want
        assert want % 16 == 0


def test_mxfp8_needs_reduce_mode():
    """dtype="mxfp8" with sum or assign raises ValueError before the
    handler (and with it the GPU) is touched: no HBM pool exists here."""
    _PORT[0] += 7
    ps.setup_env(1, 1, root_port=_PORT[0])
    roles = ("scheduler", "server", "worker")
    ths = [threading.Thread(target=ps.start, kwargs=dict(role=r, device=-1)) for r in roles]
    [t.start() for t in ths]
    [t.join() for t in ths]
    try:
        server = ps.KVServer(0)
        for mode in ("sum", "assign"):
            with pytest.raises(ValueError, match="mxfp8"):
                server.set_gpu_dense_handle(mode=mode, dtype="mxfp8")
        server.set_default_handle()
    finally:
        ths = [threading.Thread(target=ps.finalize, kwargs=dict(role=r)) for r in roles]
        [t.start() for t in ths]
        [t.join() for t in ths]
        ps.clear_registry()


def test_gradsync_rejects_bad_compress():
    from ps_lite_amd.parallel.dp import PSGradSync

    with pytest.raises(ValueError):
        PSGradSync(ps, None, [], num_workers=1, device=-1, compress="mxfp8")
    with pytest.raises(ValueError):
        PSGradSync(ps, None, [], num_workers=1, device=0, mode="sum", compress="mxfp8")
    with pytest.raises(ValueError):
        PSGradSync(ps, None, [], num_workers=1, device=0, compress="fp4")
