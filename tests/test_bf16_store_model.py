"""tests/bf16_store_model.py against things that are not the kernels: SplitMix64's published
first outputs, torch's CPU bfloat16 cast, and the store rule's own arithmetic counted out over
every 16-bit field."""
import numpy as np
import pytest
import torch

import bf16_store_model as model


def _bits(*u32):
    return np.array(u32, dtype=np.uint32).view(np.float32)


def test_mix64_is_splitmix64():
    """SplitMix64 seeded with 0 adds phi to its state and finalizes: its first three outputs"""
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert [model.mix64(k * model.PHI) for k in (1, 2, 3)] == want
    assert model.launch_seed(0, 1) == want[1] and model.row_key(0, 2) == want[2]
    assert model.launch_seed(2 ** 64 - 1, 0) == model.mix64(model.PHI - 1)  # the sum wraps


def test_r16_is_the_stated_field():
    """the vectorized fields against the three lines of the rule in Python ints"""
    rows, L = [0, 5, 63, 2 ** 40], 11
    for seed in (0, 3, 2 ** 64 - 1):
        got = model.r16(seed, rows, L)
        assert got.shape == (len(rows), L) and got.dtype == np.uint32
        for i, row in enumerate(rows):
            key = model.mix64(seed + (row + 1) * model.PHI)
            for e in range(L):
                word = model.mix64(key + (e // 4 + 1) * model.PHI)
                assert got[i, e] == (word >> 16 * (e % 4)) & 0xFFFF
    assert len(set(model.r16(0, [0], 8)[0].tolist())) == 8  # four fields a word, two words


def test_nearest_is_torch_bfloat16():
    rng = np.random.default_rng(1)
    u = rng.integers(0, 1 << 32, (1 << 20) + (1 << 14), dtype=np.uint64).astype(np.uint32)
    u = u[(u & 0x7F800000) != 0x7F800000]  # finite
    assert u.size >= 1 << 20
    # both ties: to the even high half it has, up from an odd one; with their negatives
    ties = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x00008000, 0x00018000],
                    dtype=np.uint32)
    x = np.concatenate([u, ties]).view(np.float32)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = model.store(x)
    assert np.array_equal(got, want)
    assert got[-6:].tolist() == [0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x0000, 0x0002]
    assert np.array_equal(model.widen(got).view(np.uint32), got.astype(np.uint32) << 16)


@pytest.mark.parametrize("u", [0x3F800001, 0x3F804000, 0x3F81C000, 0xBF80FFFF, 0xC0490FDB, 0x80000001,
                               0x00012345, 0x3FFF8000, 0x7F7F0001])
def test_stochastic_is_unbiased_by_counting(u):
    """over all 65536 fields the magnitude goes up for exactly u & 0xffff of them"""
    r = np.arange(1 << 16, dtype=np.uint32)
    got = model.store(np.full(r.size, u, dtype=np.uint32).view(np.float32), r)
    down, up = u >> 16, (u >> 16) + 1
    assert np.isin(got, [down, up]).all()
    assert int((got == up).sum()) == u & 0xFFFF
    assert np.array_equal(got == up, r >= (1 << 16) - (u & 0xFFFF))  # the top fields carry


@pytest.mark.parametrize("u", [0x3F800000, 0xBF810000, 0x00000000, 0x80000000, 0x7F7F0000, 0x00010000,
                               0x7F800000, 0xFF800000])
def test_a_bf16_never_moves(u):
    r = np.arange(1 << 16, dtype=np.uint32)
    x = np.full(r.size, u, dtype=np.uint32).view(np.float32)
    assert (model.store(x, r) == u >> 16).all() and model.store(x[:1])[0] == u >> 16


def test_carries_and_specials():
    r = np.arange(1 << 16, dtype=np.uint32)
    # a carry out of the mantissa lands in the exponent: 2 - 2^-24 becomes 2.0
    assert model.store(_bits(0x3FFFFFFF))[0] == 0x4000
    assert model.store(_bits(0x3FFF8000))[0] == 0x4000  # the tie at an odd high half
    assert model.store(_bits(0x3FFFFFFF), [1])[0] == 0x4000
    assert model.store(_bits(0x3FFFFFFF), [0])[0] == 0x3FFF
    # the largest finite values round to Inf
    assert model.store(_bits(0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000)).tolist() == [0x7F80, 0x7F80, 0xFF80]
    assert model.store(_bits(0x7F7F7FFF))[0] == 0x7F7F
    got = model.store(np.full(r.size, 0x7F7F8000, dtype=np.uint32).view(np.float32), r)
    assert (got[:0x8000] == 0x7F7F).all() and (got[0x8000:] == 0x7F80).all()
    # Inf and NaN see no field; a NaN whose mantissa lies in the low half alone keeps bit 0x40
    nan = _bits(0x7FC00000, 0x7F800001, 0x7F80FFFF, 0xFFC12345, 0x7F810000, 0xFF800001)
    want = [0x7FC0, 0x7FC0, 0x7FC0, 0xFFC1, 0x7F81, 0xFFC0]
    for fields in (None, np.zeros(6, np.uint32), np.full(6, 0xFFFF, np.uint32)):
        got = model.store(nan, fields)
        assert got.tolist() == want and np.isnan(model.widen(got)).all()
        inf = model.store(_bits(0x7F800000, 0xFF800000), None if fields is None else fields[:2])
        assert inf.tolist() == [0x7F80, 0xFF80]


def test_steps_in_fp32_by_hand():
    """one element each, every operation written out"""
    f = np.float32
    w, g, s, lr, eps = f(0.5), f(0.25), f(0.3), f(0.05), f(1e-6)
    x, s2 = model.adagrad_step([[w]], [[s]], [[g]], lr, eps, False)
    assert s2[0, 0] == f(s + f(g * g)) and x[0, 0] == f(w - f(f(lr * g) / f(np.sqrt(s2[0, 0]) + eps)))
    x, s2 = model.adagrad_step([[w, w]], [s], [[g, -g]], lr, eps, True)
    assert s2[0] == f(s + f(f(0.125) / f(2))) and x.dtype == np.float32
    rec = np.array([[0.5, 0.25, 0.7, 0.0, 0.1, 0.9]], dtype=np.float32)
    x, out = model.lazy_adam_step([[w]], rec, [[g]], lr, 0.5, 0.5, eps, False)
    m, v = f(f(0.5) * f(0.1) + f(0.5) * g), f(f(0.5) * f(0.9) + f(0.5) * f(g * g))
    denom = f(np.sqrt(f(v / f(1 - f(0.125)))) + eps)
    assert out[0].tolist() == [f(0.25), f(0.125), f(0.7), 0.0, m, v]
    assert x[0, 0] == f(w - f(f(f(lr / f(0.75)) * m) / denom))
