"""The bf16-table kernels with bf16 bits on the wire (kern::Sparse* with a bf16 SparseWire) on test_sparse_bf16.py's
inputs and inside its guard bytes. Fed gradient bits b, a step leaves the table and state bits
k_sparse_*_bf16 leaves fed widen(b), and its out is those table bits; the stored values keep that
file's rule against float64 from the same inputs. Row lengths: 2 and 8 (one unit), 24 (G = 4, an
idle lane), 72 (G = 16, 9 units), 1032 (one unit past the 128 resident); a table 2 bytes off
runs the element path on a vector-shaped row."""
import itertools

import numpy as np
import pytest

import ps_lite_amd as ps
from test_sparse_adagrad import _ROWS, _U, _Dev, _keys
from test_sparse_bf16 import _bf16, _widen, step_reference, stored_ok
from test_sparse_lazy_adam import _B1, _B2, _EPS, _LR, fresh

pytestmark = pytest.mark.gpu

# (optimizer, rowwise, row_len, nrows, grid_cap, with_out, rounding, key_shift, row_base, skew):
# every row length with both optimizers and variants; nrows, grid_cap, out and rounding take turns
_CASES = [c + ((1, 5, 257)[i % 3], i & 1, bool(i & 2), ("stochastic", "nearest")[(i >> 2) & 1], 0, 0, 0)
          for i, c in enumerate(itertools.product(
              ["adagrad", "lazy_adam"], [True, False], [2, 8, 24, 72, 1032]))]
_CASES.append(("lazy_adam", True, 72, 257, 1, True, "stochastic", 48, 5, 0))
_CASES += [("adagrad", True, 64, 257, 0, True, "stochastic", 0, 0, 2),
           ("lazy_adam", False, 64, 257, 0, True, "nearest", 0, 0, 2)]


def _state(rng, opt, rowwise, row_len):
    if opt == "adagrad":
        return rng.uniform(0.01, 2.0, (_ROWS,) if rowwise else (_ROWS, row_len)).astype(np.float32)
    state = fresh(_ROWS, row_len, rowwise)  # records some steps old: p = beta^k, v in [0.01, 2]
    state[:, :2] = np.array([_B1, _B2], np.float32) ** rng.choice([0, 1, 7], size=(_ROWS, 1))
    state[:, 2] = rng.uniform(0.01, 2.0, _ROWS)
    state[:, 4:] = rng.uniform(0.01, 2.0, (_ROWS, state.shape[1] - 4))
    state[:, 4:4 + row_len] = rng.standard_normal((_ROWS, row_len))
    return state


@pytest.mark.parametrize("opt,rowwise,row_len,nrows,grid_cap,with_out,rounding,shift,base,skew", _CASES)
def test_sparse_step_bf16_wire(opt, rowwise, row_len, nrows, grid_cap, with_out, rounding, shift, base,
                               skew):
    rng = np.random.default_rng([len(opt), int(rowwise), row_len, nrows, shift])
    keys, local = _keys(rng, nrows, shift, base)
    inside, rows = local >= 0, local[local >= 0]
    bits, state = _bf16(rng.standard_normal((_ROWS, row_len))), _state(rng, opt, rowwise, row_len)
    gbits = _bf16(rng.standard_normal((nrows, row_len)))
    hyper = (_LR, _EPS) if opt == "adagrad" else (_LR, _B1, _B2, _EPS)
    kw = dict(rounding=rounding, seed=3, key_shift=shift, row_base=base, table_rows=_ROWS)

    def run(kernel, grad, out0, cap):
        tab_d, st_d, grad_d, keys_d = _Dev(bits, skew), _Dev(state), _Dev(grad), _Dev(keys)
        out_d = _Dev(out0) if with_out else None
        getattr(ps._core, kernel)(tab_d.ptr, st_d.ptr, keys_d.ptr, nrows, row_len, grad_d.ptr,
                                  out_d.ptr if with_out else 0, *hyper, rowwise, grid_cap=cap, **kw)
        assert np.array_equal(grad_d.read().view(np.uint8), grad.view(np.uint8))
        return tab_d.read(), st_d.read(), out_d.read() if with_out else None

    tab, st, out = run("k_sparse_%s_bf16_wire" % opt, gbits, np.full((nrows, row_len), 0xABAB, np.uint16),
                       grid_cap)
    want = run("k_sparse_%s_bf16" % opt, _widen(gbits), np.full((nrows, row_len), np.nan, np.float32), 0)
    assert np.array_equal(tab, want[0]) and st.tobytes() == want[1].tobytes()
    if with_out:  # the stored bits, 0x0000 for a key outside the table
        assert np.array_equal(_widen(out).view(np.uint32), want[2].view(np.uint32))
        assert np.array_equal(out, np.where(inside[:, None], tab[np.maximum(local, 0)], 0))
    w_ref, w_bound, st_ref, st_bound = step_reference(
        opt, rowwise, _widen(bits)[rows], state[rows], _widen(gbits)[inside].astype(np.float64))
    assert np.all(np.abs(st[rows] - st_ref) <= st_bound)
    assert stored_ok(_widen(tab[rows]), w_ref, w_bound, rounding)
    rest = np.setdiff1d(np.arange(_ROWS), rows)
    assert np.array_equal(tab[rest], bits[rest]) and st[rest].tobytes() == state[rest].tobytes()


@pytest.mark.parametrize("row_len,grid_cap,skew", [(2, 1, 0), (8, 0, 0), (72, 1, 0), (64, 0, 2)])
def test_gather_assign_add_bf16_wire(row_len, grid_cap, skew):
    rng = np.random.default_rng([row_len, grid_cap, skew])
    keys, local = _keys(rng, 257, 0, 0)
    inside, rows = local >= 0, local[local >= 0]
    before, src = (_bf16(rng.standard_normal(s)) for s in ((_ROWS, row_len), (257, row_len)))
    src[np.flatnonzero(inside)[0], :2] = [0x8000, 0x7F7F]  # -0.0 and the largest finite, as bits
    tab_d, src_d, keys_d = _Dev(before, skew), _Dev(src), _Dev(keys)
    out_d = _Dev(np.full((257, row_len), 0xABAB, dtype=np.uint16))
    kw = dict(table_rows=_ROWS, grid_cap=grid_cap)
    ps._core.k_sparse_scatter_assign_bf16_wire(tab_d.ptr, keys_d.ptr, 257, row_len, src_d.ptr, **kw)
    ps._core.k_sparse_gather_bf16_wire(tab_d.ptr, keys_d.ptr, 257, row_len, out_d.ptr, **kw)
    want = before.copy()
    want[rows] = src[inside]
    assert np.array_equal(tab_d.read(), want)
    assert np.array_equal(out_d.read(), np.where(inside[:, None], want[np.maximum(local, 0)], 0))
    # add: one fp32 add, then R; the bits of the fp32-wire add fed the widened values. |add| >= 4
    # keeps a sum off exact zero, where the rule's ulp is zero
    add = _bf16(rng.uniform(4, 8, (257, row_len)) * rng.choice([-1, 1], (257, row_len)))
    add_d, f32_d, ref_d = _Dev(add), _Dev(_widen(add)), _Dev(want, skew)
    ps._core.k_sparse_scatter_add_bf16_wire(tab_d.ptr, keys_d.ptr, 257, row_len, add_d.ptr, seed=9, **kw)
    ps._core.k_sparse_scatter_add_bf16(ref_d.ptr, keys_d.ptr, 257, row_len, f32_d.ptr, seed=9,
                                       table_rows=_ROWS)
    got = tab_d.read()
    assert np.array_equal(got, ref_d.read())
    total = _widen(want[rows]).astype(np.float64) + _widen(add[inside])
    assert stored_ok(_widen(got[rows]), total, _U * np.abs(total), "stochastic")
    assert np.array_equal(src_d.read(), src) and np.array_equal(add_d.read(), add)
