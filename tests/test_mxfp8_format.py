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


# ---- the edge inputs of mxfp8_model.py: model and host reference against
# the expectation stated by hand (the kernels: test_mxfp8_edges_gpu.py)

_CASES = model.encode_cases(_INPUTS["edges"])


def _packed_bytes(p):
    return torch.as_tensor(np.ascontiguousarray(p)).view(torch.uint8).reshape(-1)


def _host_d(packed, n, **kw):
    return torch.from_numpy(_core.mxfp8_dequantize_host(np.ascontiguousarray(packed.numpy()), n,
                                                        **kw))


@pytest.mark.parametrize("k", model.TIE_KS)
def test_code_ties_hold_what_they_claim(k):
    x, byte, codes = model.code_ties(k)
    assert model.in_contract(x) and x.numel() == 33 * 32
    assert float(x[x != 0].abs().min()) >= 2.0 ** -100 and float(x.abs().max()) == 448 * 2.0 ** k
    # every real block has the byte k + 127 and is scaled exactly
    mb, mc = model.quantize(x)
    assert torch.equal(mb[:33], torch.full((33,), k + 127, dtype=torch.uint8)) and not mb[33:].any()
    scaled = torch.ldexp(x, torch.tensor(-k))
    assert torch.equal(torch.ldexp(scaled, torch.tensor(k)), x)
    # the scaled values are the table, the 126 ties and their neighbours
    table = torch.from_numpy(model.E4M3_VALUES).to(torch.float32)
    mids = (table[:-1] + table[1:]) / 2
    have = set(scaled.tolist())
    for t in (table, mids, torch.nextafter(mids, torch.tensor(float("inf"))),
              torch.nextafter(mids, torch.tensor(0.0))):
        assert set(t.tolist()) <= have and set((-t).tolist()) <= have
    # stated codes: the table encoder and torch's cast agree with the
    # construction on every value, the 126 ties of either sign included
    assert np.array_equal(model.hand_codes(scaled.numpy().astype(np.float64)),
                          codes.reshape(-1).numpy())
    assert torch.equal(scaled.to(torch.float8_e4m3fn).view(torch.uint8), codes.reshape(-1))
    is_tie = torch.isin(scaled.abs(), mids)
    assert int(is_tie.sum()) == 2 * 126
    assert not (codes.reshape(-1)[is_tie] & 1).any()  # every tie went to the even code
    # a negative value that rounds to zero keeps its sign bit
    assert int((codes.reshape(-1) == 0x80).sum()) == 3  # -0.0, -(2^-10), the number below it


def test_edge_inputs_hold_what_they_claim():
    x = model.amax_placement()
    assert model.in_contract(x)
    b = torch.ldexp(x, torch.tensor(-3)).view(-1, 32)
    top = b.abs().amax(dim=1)
    assert top.tolist() == [448.0] * 8 + [449.0] * 8
    assert (b.abs() == top[:, None]).sum(dim=1).tolist() == [1] * 16  # one largest magnitude
    spots = b.abs().argmax(dim=1)
    assert spots.tolist() == list(model.AMAX_SPOTS) * 4
    signs = b[torch.arange(16), spots].sign().view(4, 4)
    assert signs.tolist() == [[1.0] * 4, [-1.0] * 4] * 2
    rest = b.clone()
    rest[torch.arange(16), spots] = 0
    assert float(rest.abs().max()) < 100  # a half without the amax scales otherwise
    byte, _ = model.hand_quantize(x)
    assert byte[:16].tolist() == [130] * 8 + [131] * 8  # 448 * 2^3 keeps the byte, 449 bumps it

    for rem in model.TAIL_LENS:
        for top in (448.0, 449.0):
            for sign in (1.0, -1.0):
                t = model.amax_in_tail(rem, top, sign)
                assert model.in_contract(t) and t.numel() % 512 == rem and t.numel() > 512
                assert float(t[-1]) == sign * top * 8 and bool((t[512:-1].abs() < 800).all())
                byte, _ = model.hand_quantize(t)
                assert int(byte[16]) == (130 if top == 448.0 else 131) and not byte[17:].any()

    e = model.contract_ends()
    assert model.in_contract(e)
    amax = e.view(-1, 32).abs().amax(dim=1)
    assert amax.tolist() == [2.0 ** -100, 2.0 ** 100, 0.0, 3.0, 2.0 ** -100, 2.0 ** 100]
    assert bool(torch.signbit(e[64:96]).all())  # the block of -0.0
    byte, codes = model.hand_quantize(e)
    assert byte[:6].tolist() == [19, 219, 0, 120, 19, 219]
    assert codes[2].tolist() == [0x80] * 32  # -0.0 keeps its sign under byte 0
    assert codes[3].tolist() == [0x7C] * 32 and codes[4].tolist() == [0xF8] * 32


@pytest.mark.parametrize("name,x,want", _CASES, ids=[c[0] for c in _CASES])
def test_edge_inputs_model_and_host_byte_for_byte(name, x, want):
    """Quantize: the model's and the host reference's packed bytes, code
    bytes included (-0 and +0 differ), against the hand-stated bytes.
    Dequantize: both against the table's values, bit for bit."""
    assert model.in_contract(x)
    n = x.numel()
    assert want.numel() == model.packed_nbytes(n)
    assert torch.equal(model.pack(*model.quantize(x)), want), "model"
    assert torch.equal(_packed_bytes(_host_q(x)), want), "host reference"
    byte, codes = model.unpack(want)
    # padding past n: zero codes under byte 0
    assert not byte[-(-n // 32):].any() and not codes.view(torch.uint8).reshape(-1)[n:].any()
    back = model.hand_decode(byte, codes.view(torch.uint8)).reshape(-1)[:n]
    assert model.same_bits_or_nan(model.dequantize(byte, codes, n), back)
    assert model.same_bits_or_nan(_host_d(want, n), back)
    # the server's no-accumulator finish, Q(D(Q(x))), stated the same way
    again = model.hand_packed(back)
    assert torch.equal(model.pack(*model.quantize(back)), again)
    assert torch.equal(_packed_bytes(_host_q(back)), again)


@pytest.mark.parametrize("byte", model.TABLE_BYTES)
def test_code_table_decode(byte):
    """All 256 codes under one scale byte: model and host reference decode
    to the table's values bit for bit, 0x7F and 0xFF to NaN."""
    packed = model.code_table(byte)
    n = 1024
    sb, codes = model.unpack(packed)
    assert set(sb.tolist()) == {byte}
    have = set(codes.view(torch.uint8).reshape(-1).tolist())
    assert have == ({0x00, 0x80} if byte == 0 else set(range(256)))
    want = model.hand_decode(sb, codes.view(torch.uint8)).reshape(-1)
    assert int(torch.isnan(want).sum()) == (0 if byte == 0 else 8)
    assert model.same_bits_or_nan(model.dequantize(sb, codes, n), want)
    third = (want.to(torch.float64) * float(np.float32(1.0 / 3.0))).to(torch.float32)
    assert model.same_bits_or_nan(model.dequantize(sb, codes, n, alpha=1.0 / 3.0), third)
    if byte:  # byte 0: the host reference reads 2^-127 there, equal on zeros only
        assert model.same_bits_or_nan(_host_d(packed, n), want)
        assert model.same_bits_or_nan(_host_d(packed, n, alpha=1.0 / 3.0), third)
    else:
        assert torch.equal(_host_d(packed, n).view(torch.int32), want.view(torch.int32))


def test_non_finite_blocks():
    """The non-finite rule on the model and the host reference: a block
    with a NaN or an infinity is byte 0xFF and 32 codes 0x7F and decodes to
    32 NaNs; every other byte of the stream is that of the finite input."""
    x, bad, blocks = model.nonfinite_stream()
    assert model.in_contract(x) and len(blocks) == 10
    finite = model.hand_packed(x)
    want = model.poisoned_packed(finite, blocks)
    assert int((want != finite).sum()) > 0
    assert torch.equal(model.pack(*model.quantize(x)), finite)
    assert torch.equal(_packed_bytes(_host_q(x)), finite)
    assert torch.equal(model.pack(*model.quantize(bad)), want), "model"
    assert torch.equal(_packed_bytes(_host_q(bad)), want), "host reference"
    assert torch.equal(model.hand_packed(bad), want)
    n = x.numel()
    byte, codes = model.unpack(want)
    clean = model.dequantize(*model.unpack(finite), n)
    nan_at = torch.zeros(33 * 32, dtype=torch.bool).view(33, 32)
    nan_at[blocks] = True
    nan_at = nan_at.reshape(-1)[:n]
    for got in (model.dequantize(byte, codes, n), _host_d(want, n),
                model.dequantize(byte, codes, n, alpha=0.5) * 2, _host_d(want, n, alpha=0.5) * 2):
        assert torch.equal(torch.isnan(got), nan_at)
        assert torch.equal(got[~nan_at].view(torch.int32), clean[~nan_at].view(torch.int32))
    # the sum of a finish counts too: a finite sum that overflows fp32
    big = torch.full((32,), 3e38)
    assert bool(torch.isfinite(big).all())
    over = model.pack(*model.quantize(model.pad_super(big + big)))
    assert int(over[0]) == 0xFF and set(over[16:48].tolist()) == {0x7F} and not over[1:16].any()
    assert torch.equal(_packed_bytes(_host_q(model.pad_super(big + big))), over)


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
