"""Torch-tensor wrappers over the CDNA4 sparse row kernels."""

from .. import _core


def sparse_gather(table, rows, out=None):
    """out[i] = table[rows[i]] for a 2-D fp32 table; rows int64/uint64."""
    import torch

    assert table.is_cuda and table.dim() == 2 and table.is_contiguous()
    assert rows.is_cuda and rows.dim() == 1
    if out is None:
        out = torch.empty(rows.numel(), table.shape[1], device=table.device,
                          dtype=table.dtype)
    _core.k_sparse_gather_f32(table.data_ptr(), rows.data_ptr(), rows.numel(),
                              table.shape[1], out.data_ptr())
    return out


def sparse_scatter_add(table, rows, src, atomic=False):
    """table[rows[i]] += src[i]; atomic=True tolerates duplicate rows."""
    assert table.is_cuda and table.dim() == 2 and table.is_contiguous()
    assert src.shape == (rows.numel(), table.shape[1])
    _core.k_sparse_scatter_add_f32(table.data_ptr(), rows.data_ptr(), rows.numel(),
                                   table.shape[1], src.data_ptr(), atomic)
    return table


def sparse_adagrad(table, state, rows, grad, lr, eps=1e-8, out=None):
    """One Adagrad step on table[rows[i]] with gradient grad[i], in one launch.

    Row-wise when state.dim() == 1 (state[row] += mean(g * g)), element-wise
    when state has the table's shape (state[row] += g * g); then
    table[row] -= lr * g / (sqrt(state) + eps). Rows must be unique; a row
    outside the table is skipped. With `out` the new rows are also written
    to out[i] (zeros for a skipped row). Returns out, or table without one."""
    assert table.is_cuda and table.dim() == 2 and table.is_contiguous()
    assert state.is_cuda and state.is_contiguous()
    rowwise = state.dim() == 1
    assert state.shape == ((table.shape[0],) if rowwise else table.shape)
    assert rows.is_cuda and rows.dim() == 1
    assert grad.is_contiguous() and grad.shape == (rows.numel(), table.shape[1])
    assert out is None or (out.is_contiguous() and out.shape == grad.shape)
    _core.k_sparse_adagrad_f32(table.data_ptr(), state.data_ptr(), rows.data_ptr(),
                               rows.numel(), table.shape[1], grad.data_ptr(),
                               0 if out is None else out.data_ptr(), lr, eps, rowwise,
                               table_rows=table.shape[0])
    return table if out is None else out
