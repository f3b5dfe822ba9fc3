"""The bf16-table kernels (csrc/sparse_table.hip) against numpy float64 from the same inputs, on
test_sparse_adagrad.py's keys and inside its guard bytes. A step's fp32 result x obeys the fp32
tests' bound against the reference; the stored s = R(x) adds the rounding: |s - ref| <= ulp / 2 +
bound under nearest, < ulp + bound under stochastic, ulp = 2^(floor(log2(max(|s|, |ref|))) - 7).
The state stays fp32 and keeps the fp32 bounds. 1032 is the first multiple of 8 past the 1024
elements a wave's registers hold (the streaming tail; 130 elements on the scalar path)."""
import itertools

import numpy as np
import pytest

import ps_lite_amd as ps
from test_sparse_adagrad import _ROWS, _U, _Dev, _keys
from test_sparse_lazy_adam import _B1, _B2, _EPS, _LR, fresh, reference

pytestmark = pytest.mark.gpu

# (optimizer, rowwise, row_len, nrows, grid_cap, with_out, rounding, key_shift, row_base, skew):
# every shape with both optimizers and variants; grid_cap, out and the rounding take turns
_CASES = [c + (i & 1, bool(i & 2), ("stochastic", "nearest")[(i >> 2) & 1], 0, 0, 0)
          for i, c in enumerate(itertools.product(
              ["adagrad", "lazy_adam"], [True, False], [1, 3, 8, 20, 64, 72, 1032], [1, 5, 257]))]
_CASES.append(("lazy_adam", True, 64, 257, 1, True, "stochastic", 48, 5, 0))
# the table 2 bytes off: the scalar path on a vector-shaped row, with and without its tail
_CASES += [(o, r, n, 257, 0, True, "stochastic", 0, 0, 2)
           for o, r, n in [("adagrad", True, 64), ("lazy_adam", False, 64), ("lazy_adam", True, 1032)]]


def _bf16(x):
    """round-to-nearest-even bf16 bits of finite fp32 values"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _widen(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def _step(opt, rowwise, row_len, nrows, grid_cap, with_out, rounding, shift, base, skew, seed=3):
    """One launch on fixed inputs; returns them and what the launch left."""
    rng = np.random.default_rng([len(opt), int(rowwise), row_len, nrows, shift])
    keys, local = _keys(rng, nrows, shift, base)
    ins = np.flatnonzero(local >= 0)
    bits = _bf16(rng.standard_normal((_ROWS, row_len)))
    grad = rng.standard_normal((nrows, row_len)).astype(np.float32)
    if opt == "adagrad":
        state = rng.uniform(0.01, 2.0, (_ROWS,) if rowwise else (_ROWS, row_len)).astype(np.float32)
    else:  # test_sparse_lazy_adam.py's records: p = beta^k, v in [0.01, 2], m normal
        state = fresh(_ROWS, row_len, rowwise)
        steps = rng.choice([0, 1, 7], size=_ROWS)
        for i in range(7):
            state[steps > i, :2] *= np.array([_B1, _B2], np.float32)
        state[:, 2:] = rng.uniform(0.01, 2.0, (_ROWS, state.shape[1] - 2))
        state[:, 3], state[:, 4:4 + row_len] = 0.0, rng.standard_normal((_ROWS, row_len))
        state[local[ins[0]]] = fresh(1, row_len, rowwise)[0]
    grad[ins[0]] = 0.0  # a zero gradient (lazy Adam: on a fresh row) keeps the weight's bits
    tab_d, st_d, grad_d, keys_d = _Dev(bits, skew), _Dev(state), _Dev(grad), _Dev(keys)
    out_d = _Dev(np.full((nrows, row_len), np.nan, dtype=np.float32)) if with_out else None
    hyper = (_LR, _EPS) if opt == "adagrad" else (_LR, _B1, _B2, _EPS)
    getattr(ps._core, "k_sparse_%s_bf16" % opt)(
        tab_d.ptr, st_d.ptr, keys_d.ptr, nrows, row_len, grad_d.ptr, out_d.ptr if with_out else 0,
        *hyper, rowwise, rounding=rounding, seed=seed, key_shift=shift, row_base=base,
        table_rows=_ROWS, grid_cap=grid_cap)
    assert np.array_equal(grad_d.read().view(np.uint32), grad.view(np.uint32))
    assert np.array_equal(keys_d.read(), keys)
    return dict(local=local, ins=ins, bits=bits, grad=grad, state=state, tab=tab_d.read(),
                st=st_d.read(), out=out_d.read() if with_out else None)


def stored_ok(s, ref, bound, rounding):
    """the rule above for a stored bf16 s (widened) against the float64 reference and its bound"""
    with np.errstate(divide="ignore"):
        ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(s), np.abs(ref)))) - 7)
    err = np.abs(s.astype(np.float64) - ref)
    return bool(np.all(err <= ulp / 2 + bound) if rounding == "nearest" else np.all(err < ulp + bound))


def step_reference(opt, rowwise, w, state, g, **carried):
    """(w', its bound, state', its bound) of one float64 step with the fp32 tests' bounds:
    test_sparse_lazy_adam.py's reference, or test_sparse_adagrad.py's formulas"""
    if opt == "lazy_adam":
        return reference(w, state, g, _LR, rowwise, **carried)
    L = g.shape[1] if rowwise else 1
    s_ref = state.astype(np.float64) + ((g * g).sum(axis=1) / g.shape[1] if rowwise else g * g)
    step = _LR * g / (np.sqrt(s_ref[:, None] if rowwise else s_ref) + _EPS)
    w_ref = w.astype(np.float64) - step
    return w_ref, _U * (np.abs(w_ref) + (L / 2 + 5) * np.abs(step)), s_ref, (L + 3) * _U * np.abs(s_ref)


@pytest.mark.parametrize("opt,rowwise,row_len,nrows,grid_cap,with_out,rounding,shift,base,skew", _CASES)
def test_sparse_step_bf16(opt, rowwise, row_len, nrows, grid_cap, with_out, rounding, shift, base, skew):
    r = _step(opt, rowwise, row_len, nrows, grid_cap, with_out, rounding, shift, base, skew)
    local, inside = r["local"], r["local"] >= 0
    rows, g, w = local[inside], r["grad"][inside].astype(np.float64), _widen(r["bits"])
    w_ref, w_bound, st_ref, st_bound = step_reference(opt, rowwise, w[rows], r["state"][rows], g)
    # the records' zero bounds make p1', p2' and the rest of a lazy-Adam header exact
    assert np.all(np.abs(r["st"][rows] - st_ref) <= st_bound)
    assert stored_ok(_widen(r["tab"][rows]), w_ref, w_bound, rounding)
    still = np.append(np.setdiff1d(np.arange(_ROWS), rows), local[r["ins"][0]])
    assert np.array_equal(r["tab"][still], r["bits"][still])
    rest = np.setdiff1d(np.arange(_ROWS), rows)
    assert np.array_equal(r["st"][rest].view(np.uint32), r["state"][rest].view(np.uint32))
    if with_out:  # what a gather returns bit for bit, zeros for a key outside the table
        want = np.where(inside[:, None], _widen(r["tab"][np.maximum(local, 0)]).view(np.uint32), 0)
        assert np.array_equal(r["out"].view(np.uint32), want)


@pytest.mark.parametrize("opt,rowwise", [("adagrad", True), ("lazy_adam", False)])
def test_same_seed_same_bits(opt, rowwise):
    def tab(grid_cap, skew, seed):
        return _step(opt, rowwise, 64, 257, grid_cap, True, "stochastic", 0, 0, skew, seed)["tab"]
    first = tab(0, 0, 7)
    assert np.array_equal(first, tab(1, 0, 7)) and np.array_equal(first, tab(0, 2, 7))
    assert not np.array_equal(first, tab(0, 0, 8))


@pytest.mark.parametrize("row_len,grid_cap,skew", [(1, 1, 0), (3, 0, 0), (8, 1, 0), (72, 0, 0), (64, 0, 2)])
def test_assign_and_gather_bf16(row_len, grid_cap, skew):
    rng = np.random.default_rng([row_len, grid_cap, skew])
    keys, local = _keys(rng, 257, 0, 0)
    inside, rows = local >= 0, local[local >= 0]
    src = rng.standard_normal((257, row_len)).astype(np.float32)
    # ties to even both ways, up across a binade (2 - 2^-8 is the tie below 2), inf, -0
    edge = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1.999, -(2 - 2.0 ** -8) - 2.0 ** -9, np.inf,
                     -0.0], dtype=np.float32)[:row_len]
    first = np.flatnonzero(inside)[0]
    src[first, :len(edge)] = edge
    before = _bf16(rng.standard_normal((_ROWS, row_len)))
    tab_d, src_d, keys_d = _Dev(before, skew), _Dev(src), _Dev(keys)
    out_d = _Dev(np.full((257, row_len), np.nan, dtype=np.float32))
    kw = dict(table_rows=_ROWS, grid_cap=grid_cap)
    ps._core.k_sparse_scatter_assign_bf16(tab_d.ptr, keys_d.ptr, 257, row_len, src_d.ptr, **kw)
    ps._core.k_sparse_gather_bf16(tab_d.ptr, keys_d.ptr, 257, row_len, out_d.ptr, **kw)
    want = before.copy()
    want[rows] = _bf16(src[inside])
    got = tab_d.read()
    by_hand = [0x3F80, 0x3F82, 0x4000, 0xC000, 0x7F80, 0x8000][:row_len]
    assert got[local[first], :len(edge)].tolist() == by_hand
    assert np.array_equal(got, want)
    gathered = np.where(inside[:, None], _widen(want[np.maximum(local, 0)]).view(np.uint32), 0)
    assert np.array_equal(out_d.read().view(np.uint32), gathered)
    assert np.array_equal(src_d.read().view(np.uint32), src.view(np.uint32))


@pytest.mark.parametrize("f", [1 / 4, 1 / 2, 13 / 16])
def test_stochastic_rounding_is_unbiased(f):
    """1 + f * 2^-7 is exact in fp32 and lies f of the way from 1.0 to the next bf16."""
    n, L = 4096, 64
    tab_d = _Dev(np.full((n, L), 0x3F80, dtype=np.uint16))
    src_d = _Dev(np.full((n, L), f * 2.0 ** -7, dtype=np.float32))
    keys_d = _Dev(np.arange(n, dtype=np.uint64))
    ps._core.k_sparse_scatter_add_bf16(tab_d.ptr, keys_d.ptr, n, L, src_d.ptr, rounding="stochastic",
                                       seed=11, table_rows=n)
    got = tab_d.read()
    assert np.isin(got, [0x3F80, 0x3F81]).all()
    up = got == 0x3F81
    print("share rounded up: %.5f, columns %.4f..%.4f" % (up.mean(), up.mean(0).min(), up.mean(0).max()))
    assert abs(up.mean() - f) <= 5 * np.sqrt(f * (1 - f) / up.size)
    assert np.all(np.abs(up.mean(axis=0) - f) <= 5 * np.sqrt(f * (1 - f) / n))
