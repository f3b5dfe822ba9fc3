"""kern::SparseCoalesceBf16 (csrc/sparse_coalesce.hip): keys and inverse are the fp32 call's, the
sums are np.add.at on a zero fp32 array rounded once to nearest even, bit for bit, and rows past m
keep their bytes. Row lengths 2 (elements), 8 and 72 (16 B stores); n up to one past the tile."""
import numpy as np
import pytest

import ps_lite_amd as ps
from ps_lite_amd import ops
from test_sparse_bf16 import _bf16
from test_sparse_coalesce import _Dev

pytestmark = pytest.mark.gpu

_T = ps._core.coalesce_tile


@pytest.mark.parametrize("n,row_len,grad_rows,grid_cap", [
    (1, 2, 1, 0), (7, 8, 7, 1), (7, 72, 4, 0), (_T + 1, 2, _T + 1, 1), (_T + 1, 8, _T + 1, 0),
    (_T + 1, 72, _T + 1, 1)])
def test_sparse_coalesce_bf16_sums(n, row_len, grad_rows, grid_cap):
    rng = np.random.default_rng([n, row_len, grad_rows])
    ids = rng.choice(rng.choice(1 << 20, 5, replace=False), n).astype(np.uint64)  # heavy repetition
    grad = (rng.standard_normal((grad_rows, row_len)) * 10.0 ** rng.integers(-3, 4, (grad_rows, 1))
            ).astype(np.float32)
    ws_bytes = ps._core.sparse_coalesce_workspace_bytes(n)
    ids_d, grad_d, ws_d = _Dev(ids), _Dev(grad), _Dev(np.zeros(ws_bytes, dtype=np.uint8))

    def run(sums0, **kw):
        keys_d, sums_d, inv_d = _Dev(np.zeros(n, np.uint64)), _Dev(sums0), _Dev(np.full(n, -1, np.int64))
        m = ps._core.k_sparse_coalesce(ids_d.ptr, n, 3, grad_d.ptr, grad_rows, row_len, keys_d.ptr,
                                       sums_d.ptr, inv_d.ptr, ws_d.ptr, ws_bytes, grid_cap=grid_cap, **kw)
        return m, keys_d.read(), inv_d.read(), sums_d.read()

    sums0 = np.full((n, row_len), 0xABAB, dtype=np.uint16)
    m, keys, inverse, sums = run(sums0, sums_bf16=True)
    m32, keys32, inverse32, _ = run(np.zeros((n, row_len), np.float32))
    assert m == m32 == np.unique(ids).size
    assert np.array_equal(keys, keys32) and np.array_equal(inverse, inverse32)
    want = np.zeros((m, row_len), dtype=np.float32)
    np.add.at(want, inverse[:grad_rows], grad)
    assert np.array_equal(sums[:m], _bf16(want))
    assert np.array_equal(sums[m:], sums0[m:])
    assert np.array_equal(grad_d.read().view(np.uint32), grad.view(np.uint32))
    ws_d.read()  # the workspace's guard bytes


def test_ops_coalesce_and_gather_bf16():
    """the worker's two ends of a 16-bit round: bf16 sums out, fp32 rows per occurrence back"""
    import torch
    rng = np.random.default_rng(5)
    ids = torch.from_numpy(rng.integers(0, 9, 40)).to("cuda:0")
    grad = torch.from_numpy(rng.standard_normal((40, 8)).astype(np.float32)).to("cuda:0")
    keys, sums, inverse = ops.sparse_coalesce(ids, grad, sums_dtype=torch.bfloat16)
    want = np.zeros((keys.numel(), 8), dtype=np.float32)
    np.add.at(want, inverse.cpu().numpy(), grad.cpu().numpy())
    assert sums.dtype == torch.bfloat16
    assert np.array_equal(sums.view(torch.int16).cpu().numpy().view(np.uint16), _bf16(want))
    rows = ops.sparse_gather(sums, inverse)
    assert rows.dtype == torch.float32 and torch.equal(rows, sums.float()[inverse])
