"""Torch-tensor wrappers over the CDNA4 sparse row kernels."""

from .. import _core


def sparse_gather(table, rows, out=None):
    """out[i] = table[rows[i]] for a 2-D fp32 table; rows int64/uint64.

    A torch.bfloat16 table gives fp32 rows, widened exactly: how the rows of
    a 16-bit pull response become one fp32 row per occurrence."""
    import torch

    assert table.is_cuda and table.dim() == 2 and table.is_contiguous()
    assert rows.is_cuda and rows.dim() == 1
    if out is None:
        out = torch.empty(rows.numel(), table.shape[1], device=table.device,
                          dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous()
    gather = _core.k_sparse_gather_bf16 if _is_bf16(table) else _core.k_sparse_gather_f32
    gather(table.data_ptr(), rows.data_ptr(), rows.numel(), table.shape[1], out.data_ptr())
    return out


def sparse_scatter_add(table, rows, src, atomic=False):
    """table[rows[i]] += src[i]; atomic=True tolerates duplicate rows."""
    assert table.is_cuda and table.dim() == 2 and table.is_contiguous()
    assert src.shape == (rows.numel(), table.shape[1])
    _core.k_sparse_scatter_add_f32(table.data_ptr(), rows.data_ptr(), rows.numel(),
                                   table.shape[1], src.data_ptr(), atomic)
    return table


def sparse_coalesce(ids, grad=None, key_shift=0, out_keys=None, out_sums=None, workspace=None,
                    sums_dtype=None):
    """Sorted unique keys, summed gradient rows and the slot of every id.

    ids: int64 or uint64 CUDA tensor of any shape, any order, any repetition
    (compared as unsigned). grad: (grad_rows, row_len) fp32, row i for
    ids.flatten()[i]; ids past grad_rows carry no gradient. Returns
    (keys[:m], sums[:m] or None, inverse): keys ascending, each
    id << key_shift; sums[u] the rows of key u added in ascending i, bit for
    bit the same on every run; inverse int64 with inverse[i] the slot of id i.
    out_keys (>= n elements), out_sums (>= n rows of row_len) and workspace
    (>= _core.sparse_coalesce_workspace_bytes(n) bytes) are optional
    preallocated buffers; with all three nothing but inverse is allocated.
    A torch.bfloat16 out_sums, or sums_dtype=torch.bfloat16 without one,
    gives each fp32 sum rounded once to nearest even: the rows a handler with
    wire_dtype="bf16" takes."""
    import torch

    assert ids.is_cuda and ids.dtype in (torch.int64, torch.uint64)
    ids = ids.reshape(-1)  # a view of a contiguous tensor
    n = ids.numel()
    grad_rows, row_len = (0, 0) if grad is None else grad.shape
    if grad is not None:
        assert grad.is_cuda and grad.dtype == torch.float32 and grad.is_contiguous()
        if out_sums is None:
            out_sums = torch.empty(n, row_len, device=ids.device,
                                   dtype=sums_dtype or torch.float32)
        assert out_sums.is_contiguous() and out_sums.dtype in (torch.float32, torch.bfloat16)
        assert sums_dtype in (None, out_sums.dtype)
        assert out_sums.dim() == 2 and out_sums.shape[0] >= n and out_sums.shape[1] == row_len
    if out_keys is None:
        out_keys = torch.empty(n, device=ids.device, dtype=ids.dtype)
    assert out_keys.is_contiguous() and out_keys.numel() >= n and out_keys.element_size() == 8
    need = _core.sparse_coalesce_workspace_bytes(n)
    if workspace is None:
        workspace = torch.empty(need, device=ids.device, dtype=torch.uint8)
    ws_bytes = workspace.numel() * workspace.element_size()
    inverse = torch.empty(n, device=ids.device, dtype=torch.int64)
    m = _core.k_sparse_coalesce(ids.data_ptr(), n, key_shift,
                                0 if grad is None else grad.data_ptr(), grad_rows, row_len,
                                out_keys.data_ptr(), 0 if grad is None else out_sums.data_ptr(),
                                inverse.data_ptr(), workspace.data_ptr(), ws_bytes,
                                sums_bf16=grad is not None and _is_bf16(out_sums))
    return out_keys[:m], (None if grad is None else out_sums[:m]), inverse


def _is_bf16(table):
    import torch

    return table.dtype == torch.bfloat16


def sparse_adagrad(table, state, rows, grad, lr, eps=1e-8, out=None, rounding="stochastic",
                   seed=0):
    """One Adagrad step on table[rows[i]] with gradient grad[i], in one launch.

    Row-wise when state.dim() == 1 (state[row] += mean(g * g)), element-wise
    when state has the table's shape (state[row] += g * g); then
    table[row] -= lr * g / (sqrt(state) + eps). Rows must be unique; a row
    outside the table is skipped. With `out` the new rows are also written
    to out[i] (zeros for a skipped row). Returns out, or table without one.

    A torch.bfloat16 table (state, grad and out stay fp32) runs the same fp32
    arithmetic and rounds once on the store: rounding="stochastic" (seeded by
    `seed`; pass a new one every step) or "nearest"; out then holds the stored
    values widened to fp32."""
    assert table.is_cuda and table.dim() == 2 and table.is_contiguous()
    assert state.is_cuda and state.is_contiguous()
    rowwise = state.dim() == 1
    assert state.shape == ((table.shape[0],) if rowwise else table.shape)
    assert rows.is_cuda and rows.dim() == 1
    assert grad.is_contiguous() and grad.shape == (rows.numel(), table.shape[1])
    assert out is None or (out.is_contiguous() and out.shape == grad.shape)
    args = (table.data_ptr(), state.data_ptr(), rows.data_ptr(), rows.numel(), table.shape[1],
            grad.data_ptr(), 0 if out is None else out.data_ptr(), lr, eps, rowwise)
    if _is_bf16(table):
        _core.k_sparse_adagrad_bf16(*args, rounding=rounding, seed=seed,
                                    table_rows=table.shape[0])
    else:
        _core.k_sparse_adagrad_f32(*args, table_rows=table.shape[0])
    return table if out is None else out


def sparse_lazy_adam_state(table, rowwise=False):
    """A fresh lazy-Adam state for `table` (fp32 or bf16): a flat fp32 tensor of one record
    per row, {p1, p2, v_row, 0} m[row_len] and, element-wise only, v[row_len],
    with p1 = p2 = 1 and zeros everywhere else."""
    import torch

    rows, row_len = table.shape
    state = torch.zeros(_core.sparse_lazy_adam_state_floats(rows, row_len, rowwise),
                        device=table.device, dtype=torch.float32)
    state.view(rows, -1)[:, :2] = 1.0
    return state


def sparse_lazy_adam(table, state, rows, grad, lr, beta1=0.9, beta2=0.999, eps=1e-8,
                     rowwise=False, out=None, rounding="stochastic", seed=0):
    """One sparse Adam step on table[rows[i]] with gradient grad[i], in one launch.

    The bias correction is each row's own: its record in `state`
    (sparse_lazy_adam_state) carries p1 = beta1^t and p2 = beta2^t over the
    steps that row has taken. m = beta1 * m + (1 - beta1) * g; v = beta2 * v +
    (1 - beta2) * g * g per element, or with rowwise one v per row from
    mean(g * g); then table[row] -= lr / (1 - p1) * m / (sqrt(v / (1 - p2)) +
    eps). Rows must be unique; a row outside the table is skipped. With `out`
    the new rows are also written to out[i] (zeros for a skipped row).
    Returns out, or table without one. A torch.bfloat16 table takes `rounding`
    and `seed` as sparse_adagrad does."""
    assert table.is_cuda and table.dim() == 2 and table.is_contiguous()
    assert state.is_cuda and state.dim() == 1 and state.is_contiguous()
    assert state.numel() == _core.sparse_lazy_adam_state_floats(*table.shape, rowwise)
    assert rows.is_cuda and rows.dim() == 1
    assert grad.is_contiguous() and grad.shape == (rows.numel(), table.shape[1])
    assert out is None or (out.is_contiguous() and out.shape == grad.shape)
    args = (table.data_ptr(), state.data_ptr(), rows.data_ptr(), rows.numel(), table.shape[1],
            grad.data_ptr(), 0 if out is None else out.data_ptr(), lr, beta1, beta2, eps, rowwise)
    if _is_bf16(table):
        _core.k_sparse_lazy_adam_bf16(*args, rounding=rounding, seed=seed,
                                      table_rows=table.shape[0])
    else:
        _core.k_sparse_lazy_adam_f32(*args, table_rows=table.shape[0])
    return table if out is None else out
