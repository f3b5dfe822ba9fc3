"""kern::SparseCoalesce (csrc/sparse_coalesce.hip) against numpy: m, the keys and the inverse
equal np.unique's, the sums equal np.add.at on a zero fp32 array bit for bit (the same adds in
the same order) and lie within (k - 1) * 2^-23 * sum|g| of the float64 sum, k the key's
gradient rows: the bound of a sequential sum. Every buffer lies inside 0xAB guard bytes; ids,
grad and the slots past m keep their bytes."""
import numpy as np
import pytest

import ps_lite_amd as ps

pytestmark = pytest.mark.gpu

_T, _PAD = ps._core.coalesce_tile, 64
_SIZES = [(1, 0), (2, 0), (65, 0), (_T, 0), (_T + 1, 0), (3 * _T + 5, 0), (5 * _T + 3, 1)]
_PATTERNS = ["equal", "descending", "pool37", "extremes", "halves"]
_N = 3 * _T + 5
# (n, grid_cap, ids, row_len, grad_rows or None for no gradient, key_shift, skew bytes)
_CASES = [(n, cap, p, 4, n, 0, 0) for n, cap in _SIZES for p in _PATTERNS]
_CASES += [(_N, 0, "pool37", row_len, _N, 0, 0) for row_len in (1, 3, 20, 260)]
_CASES += [(_N, 0, "pool37", 4, rows, 0, 0) for rows in (_N // 2, 0, None)]
_CASES += [(_N, 0, "pool37", 4, _N, 44, 0), (65, 0, "descending", 3, 65, 44, 0),
           (_N, 0, "pool37", 4, _N, 0, 4)]


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


def _ids(rng, pattern, n):
    if pattern == "equal":  # one segment across every tile and every merge cut
        return np.full(n, 7, dtype=np.uint64)
    if pattern == "descending":
        return (3 * np.arange(n, 0, -1)).astype(np.uint64)
    if pattern == "pool37":  # long segments, mostly ties in the merge; all below 2^20
        return rng.choice(rng.choice(1 << 20, 37, replace=False), n).astype(np.uint64)
    if pattern == "extremes":  # unsigned compare; a real all-ones key against the padding
        return rng.choice(np.array([1 << 63, (1 << 64) - 1, 0, (1 << 63) - 1, 1], dtype=np.uint64), n)
    low, high = rng.integers(0, 5, n, dtype=np.uint64), rng.integers(0, 5, n, dtype=np.uint64)
    return np.where(rng.random(n) < 0.5, (high << np.uint64(32)) | np.uint64(9),  # "halves"
                    (np.uint64(9) << np.uint64(32)) | low)


@pytest.mark.parametrize("n,grid_cap,pattern,row_len,grad_rows,shift,skew", _CASES)
def test_sparse_coalesce(n, grid_cap, pattern, row_len, grad_rows, shift, skew):
    rng = np.random.default_rng([n, _PATTERNS.index(pattern), row_len, grad_rows or 0, shift, skew])
    ids = _ids(rng, pattern, n)
    rows = grad_rows or 0
    grad = (rng.standard_normal((rows, row_len)) * 10.0 ** rng.integers(-3, 4, (rows, 1))
            ).astype(np.float32)
    keys0 = np.full(n, 0xABABABABABABABAB, dtype=np.uint64)
    sums0 = np.full((n, row_len), np.nan, dtype=np.float32)
    ids_d, grad_d, keys_d, sums_d = _Dev(ids), _Dev(grad, skew), _Dev(keys0), _Dev(sums0, skew)
    inv_d = _Dev(np.full(n, -1, dtype=np.int64))
    ws_bytes = ps._core.sparse_coalesce_workspace_bytes(n)
    ws_d = _Dev(np.zeros(ws_bytes, dtype=np.uint8))
    m = ps._core.k_sparse_coalesce(ids_d.ptr, n, shift, 0 if grad_rows is None else grad_d.ptr,
                                   rows, row_len, keys_d.ptr, sums_d.ptr, inv_d.ptr, ws_d.ptr,
                                   ws_bytes, grid_cap=grid_cap)
    uniq, inverse = np.unique(ids, return_inverse=True)
    assert m == uniq.size
    got_keys, got_sums = keys_d.read(), sums_d.read()
    assert np.array_equal(got_keys[:m], uniq << np.uint64(shift))
    assert np.array_equal(inv_d.read(), inverse)
    want = np.zeros((m, row_len), dtype=np.float32)
    np.add.at(want, inverse[:rows], grad)
    assert np.array_equal(got_sums[:m].view(np.uint32), want.view(np.uint32))
    exact, mass = np.zeros((m, row_len)), np.zeros((m, row_len))
    np.add.at(exact, inverse[:rows], grad.astype(np.float64))
    np.add.at(mass, inverse[:rows], np.abs(grad.astype(np.float64)))
    k = np.bincount(inverse[:rows], minlength=m)[:, None]
    assert np.all(np.abs(got_sums[:m] - exact) <= np.maximum(k - 1, 0) * 2.0 ** -23 * mass)
    assert np.array_equal(got_keys[m:], keys0[m:])
    assert np.array_equal(got_sums[m:].view(np.uint32), sums0[m:].view(np.uint32))
    assert np.array_equal(ids_d.read(), ids)
    assert np.array_equal(grad_d.read().view(np.uint32), grad.view(np.uint32))
    ws_d.read()  # the workspace's guard bytes
