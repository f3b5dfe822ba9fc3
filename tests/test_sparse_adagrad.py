"""kern::SparseAdagrad on an fp32 table (csrc/sparse_table.hip) against the update in numpy float64 from the
same fp32 inputs. With every fp32 operation within u = 2^-23 relative and a sum of L squares
within L*u: |w - w_ref| <= u * (|w_ref| + (L/2 + 5) * |step_ref|) and |s - s_ref| <=
(L + 3) * u * |s_ref|, L = row_len row-wise, 1 element-wise. Table, state and out lie inside
0xAB guard bytes; whatever the call does not name keeps its bytes, gradients and keys too."""
import itertools

import numpy as np
import pytest

import ps_lite_amd as ps

pytestmark = pytest.mark.gpu

_U, _ROWS, _PAD, _TOP = 2.0 ** -23, 64, 64, (1 << 64) - 1
_LR, _EPS = float(np.float32(0.05)), float(np.float32(1e-6))
# (row_len, nrows, rowwise, grid_cap, with_out, key_shift, row_base, skew bytes)
_CASES = [c + (0, 0, 0) for c in itertools.product(
    [1, 3, 4, 20, 64, 260, 1028], [1, 5, 257], [True, False], [0, 1], [True, False])]
_CASES.append((64, 257, True, 1, True, 48, 5, 0))
# table, grad and out 4 bytes off: the scalar path on a vector-shaped row
_CASES += [(64, 257, True, 0, True, 0, 0, 4), (64, 257, False, 0, True, 0, 0, 4)]


class _Dev:
    """A device buffer: _PAD guard bytes, `skew` more, the payload, _PAD guard bytes."""

    def __init__(self, payload, skew=0):
        import torch
        self.src = np.ascontiguousarray(payload)
        self.image = np.full(2 * _PAD + skew + self.src.nbytes, 0xAB, dtype=np.uint8)
        self.at = slice(_PAD + skew, _PAD + skew + self.src.nbytes)
        self.image[self.at] = self.src.reshape(-1).view(np.uint8)
        self.dev = torch.from_numpy(self.image.copy()).to("cuda:0")
        assert self.dev.data_ptr() % 16 == 0
        self.ptr = self.dev.data_ptr() + self.at.start

    def read(self):
        got = self.dev.cpu().numpy()
        payload = got[self.at].copy()
        got[self.at] = self.image[self.at]
        assert np.array_equal(got, self.image), "guard bytes changed"
        return payload.view(self.src.dtype).reshape(self.src.shape)


def _keys(rng, nrows, shift, base):
    """(keys, local row or -1): unique rows mixed with keys at table_rows and beyond"""
    n_in = {1: 1, 5: 2}.get(nrows, 40)
    local = [int(r) for r in rng.choice(_ROWS, size=n_in, replace=False)]
    outside = [_ROWS, _ROWS + 7, _TOP] + ([-1] if base else [])
    local += [outside[i % len(outside)] for i in range(nrows - n_in)]
    rng.shuffle(local)
    keys = [r if r == _TOP else
            (((r + base) << shift) | int(rng.integers(0, 1 << shift))) & _TOP for r in local]
    return np.array(keys, dtype=np.uint64), np.array([r if 0 <= r < _ROWS else -1 for r in local])


@pytest.mark.parametrize("row_len,nrows,rowwise,grid_cap,with_out,shift,base,skew", _CASES)
def test_sparse_adagrad(row_len, nrows, rowwise, grid_cap, with_out, shift, base, skew):
    rng = np.random.default_rng([row_len, nrows, int(rowwise), grid_cap, int(with_out), shift, skew])
    keys, local = _keys(rng, nrows, shift, base)
    inside = local >= 0
    table = rng.standard_normal((_ROWS, row_len)).astype(np.float32)
    state = rng.uniform(0.01, 2.0, (_ROWS,) if rowwise else (_ROWS, row_len)).astype(np.float32)
    grad = rng.standard_normal((nrows, row_len)).astype(np.float32)
    if inside.sum() > 1:
        grad[np.flatnonzero(inside)[0]] = 0.0  # a zero gradient is a zero step
    tab_d, st_d, grad_d, keys_d = _Dev(table, skew), _Dev(state), _Dev(grad, skew), _Dev(keys)
    out_d = _Dev(np.full((nrows, row_len), np.nan, dtype=np.float32), skew) if with_out else None
    ps._core.k_sparse_adagrad_f32(tab_d.ptr, st_d.ptr, keys_d.ptr, nrows, row_len, grad_d.ptr,
                                  out_d.ptr if with_out else 0, _LR, _EPS, rowwise, key_shift=shift,
                                  row_base=base, table_rows=_ROWS, grid_cap=grid_cap)
    rows, g = local[inside], grad[inside].astype(np.float64)
    L = row_len if rowwise else 1
    s_ref = state[rows].astype(np.float64) + ((g * g).sum(axis=1) / row_len if rowwise else g * g)
    step_ref = _LR * g / (np.sqrt(s_ref[:, None] if rowwise else s_ref) + _EPS)
    w_ref = table[rows].astype(np.float64) - step_ref
    got_tab, got_st = tab_d.read(), st_d.read()
    w_err = np.abs(got_tab[rows] - w_ref) / (_U * (np.abs(w_ref) + (L / 2 + 5) * np.abs(step_ref)))
    s_err = np.abs(got_st[rows] - s_ref) / ((L + 3) * _U * np.abs(s_ref))
    print("worst error / bound: weights %.3f state %.3f" % (w_err.max(), s_err.max()))
    assert w_err.max() <= 1.0 and s_err.max() <= 1.0
    rest = np.setdiff1d(np.arange(_ROWS), rows)
    assert np.array_equal(got_tab[rest].view(np.uint32), table[rest].view(np.uint32))
    assert np.array_equal(got_st[rest].view(np.uint32), state[rest].view(np.uint32))
    assert np.array_equal(grad_d.read().view(np.uint32), grad.view(np.uint32))
    assert np.array_equal(keys_d.read(), keys)
    if with_out:  # the table's new rows bit for bit, zeros for a key outside the table
        want = np.where(inside[:, None], got_tab[np.maximum(local, 0)].view(np.uint32), 0)
        assert np.array_equal(out_d.read().view(np.uint32), want)
