"""kern::SparseLazyAdam on an fp32 table (csrc/sparse_table.hip) against the update in numpy float64 from the
same fp32 inputs, on test_sparse_adagrad.py's grid of shapes and inside its guard bytes.

Bounds from the operation order stated at the kernel: u = 2^-23 per fp32 operation, first
order, multiply-adds counted uncontracted. The fp32 p' = p * beta and 1 - beta are taken as
given (p' must match bit for bit). With a = beta1 * m, b = omb1 * g, c = omb2 * x (x = g * g, or
row-wise sum(g * g) / L: L * u for the sum, u for the division) and d = beta2 * v:
  bm = u * (|a| + |b| + |m'|)
  bv = u * (K * c + d + v'), K = 2 element-wise and L + 2 row-wise
  e(p') = u * p' / (1 - p') + (u if p' < 0.5 else 0), the relative error of 1 - p': exact for
    p' >= 0.5, else one rounding; a compiler that contracts p * beta into the subtraction uses
    the unrounded product, which moves 1 - p' by up to u * p' / (1 - p')
  bw = u * |w'| + |step| * (e(p1') + e(p2') / 2 + bv / (2 v') + 5.5 u) + lr / (1 - p1') / denom * bm
    (two divisions, a multiply, the root and the eps add: 5 u; the division under the root: u / 2)
A step from values already off by (bw, bm, bv) adds bw and takes beta1 * bm, beta2 * bv along."""
import numpy as np
import pytest

import ps_lite_amd as ps
from test_sparse_adagrad import _CASES, _ROWS, _Dev, _keys

pytestmark = pytest.mark.gpu

_U = 2.0 ** -23
_LR, _EPS = float(np.float32(0.05)), float(np.float32(1e-6))
_B = np.array([0.9, 0.999], dtype=np.float32)
_B1, _B2, _O1, _O2 = (float(x) for x in (*_B, *(np.float32(1) - _B)))


def reference(w, st, g, lr, rowwise, bw=0.0, sb=None):
    """One float64 step of n rows: weights w (n, L), state records st (n, R), gradients g, with
    the bounds bw, sb they come with. Returns (w', its bound, records', their bounds); a zero
    bound asks for the exact value."""
    L = g.shape[1]
    w, st, g = (np.asarray(x, dtype=np.float64) for x in (w, st, g))
    sb = np.zeros_like(st) if sb is None else sb
    ms, vs = slice(4, 4 + L), slice(2, 3) if rowwise else slice(4 + L, 4 + 2 * L)
    p = (st[:, :2].astype(np.float32) * _B).astype(np.float64)
    (d1, d2), (e1, e2) = (1 - p).T[:, :, None], (_U * (p / (1 - p) + (p < 0.5))).T[:, :, None]
    a, b = _B1 * st[:, ms], _O1 * g
    c = _O2 * ((g * g).sum(axis=1, keepdims=True) / L if rowwise else g * g)
    d = _B2 * st[:, vs]
    m2, v2 = a + b, c + d
    bm = _B1 * sb[:, ms] + _U * (np.abs(a) + np.abs(b) + np.abs(m2))
    bv = _B2 * sb[:, vs] + _U * ((L + 2 if rowwise else 2) * c + d + v2)
    denom = np.sqrt(v2 / d2) + _EPS
    step = lr / d1 * m2 / denom
    ev = np.divide(bv, v2, out=np.zeros_like(v2), where=v2 > 0)
    bw = bw + _U * np.abs(w - step) + np.abs(step) * (e1 + e2 / 2 + ev / 2 + 5.5 * _U) \
        + lr / d1 / denom * bm
    st2, sb2 = st.copy(), np.zeros_like(st)
    st2[:, :2], st2[:, ms], st2[:, vs] = p, m2, v2
    sb2[:, ms], sb2[:, vs] = bm, bv
    return w - step, bw, st2, sb2


def worst(got, ref, bound):
    """largest error / bound; where the bound is zero the value must be exact"""
    err = np.abs(got - ref)
    assert not err[bound == 0].any()
    return float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))


def fresh(rows, row_len, rowwise):
    state = np.zeros((rows, 4 + row_len * (1 if rowwise else 2)), dtype=np.float32)
    state[:, :2] = 1.0
    return state


@pytest.mark.parametrize("row_len,nrows,rowwise,grid_cap,with_out,shift,base,skew", _CASES)
def test_sparse_lazy_adam(row_len, nrows, rowwise, grid_cap, with_out, shift, base, skew):
    rng = np.random.default_rng([row_len, nrows, int(rowwise), grid_cap, int(with_out), shift, skew])
    keys, local = _keys(rng, nrows, shift, base)
    inside, ins = local >= 0, np.flatnonzero(local >= 0)
    table = rng.standard_normal((_ROWS, row_len)).astype(np.float32)
    grad = rng.standard_normal((nrows, row_len)).astype(np.float32)
    # records: p = beta^k as running fp32 products, k in {0, 1, 7}; v_row, v in [0.01, 2]; m normal
    state = fresh(_ROWS, row_len, rowwise)
    steps = rng.choice([0, 1, 7], size=_ROWS)
    for i in range(7):
        state[steps > i, :2] *= _B
    state[:, 2:] = rng.uniform(0.01, 2.0, (_ROWS, state.shape[1] - 2))
    state[:, 3], state[:, 4:4 + row_len] = 0.0, rng.standard_normal((_ROWS, row_len))
    if len(ins) > 2:
        grad[ins[0]] = 0.0  # a zero gradient on a row with history
    if len(ins) > 1:  # a zero gradient on a fresh row: the weight keeps its bits
        grad[ins[1]], state[local[ins[1]]] = 0.0, fresh(1, row_len, rowwise)[0]
    tab_d, st_d, grad_d, keys_d = _Dev(table, skew), _Dev(state), _Dev(grad, skew), _Dev(keys)
    out_d = _Dev(np.full((nrows, row_len), np.nan, dtype=np.float32), skew) if with_out else None
    ps._core.k_sparse_lazy_adam_f32(tab_d.ptr, st_d.ptr, keys_d.ptr, nrows, row_len, grad_d.ptr,
                                    out_d.ptr if with_out else 0, _LR, _B1, _B2, _EPS, rowwise,
                                    key_shift=shift, row_base=base, table_rows=_ROWS,
                                    grid_cap=grid_cap)
    rows = local[inside]
    w_ref, w_bound, st_ref, st_bound = reference(table[rows], state[rows], grad[inside], _LR, rowwise)
    got_tab, got_st = tab_d.read(), st_d.read()
    # the records' zero bounds make p1', p2' and the rest of the header exact
    ratios = worst(got_tab[rows], w_ref, w_bound), worst(got_st[rows], st_ref, st_bound)
    print("worst error / bound: weights %.3f state %.3f" % ratios)
    assert max(ratios) <= 1.0
    if len(ins) > 1:
        row = local[ins[1]]
        assert np.array_equal(got_tab[row].view(np.uint32), table[row].view(np.uint32))
    rest = np.setdiff1d(np.arange(_ROWS), rows)
    assert np.array_equal(got_tab[rest].view(np.uint32), table[rest].view(np.uint32))
    assert np.array_equal(got_st[rest].view(np.uint32), state[rest].view(np.uint32))
    assert np.array_equal(grad_d.read().view(np.uint32), grad.view(np.uint32))
    assert np.array_equal(keys_d.read(), keys)
    if with_out:  # the table's new rows bit for bit, zeros for a key outside the table
        want = np.where(inside[:, None], got_tab[np.maximum(local, 0)].view(np.uint32), 0)
        assert np.array_equal(out_d.read().view(np.uint32), want)
