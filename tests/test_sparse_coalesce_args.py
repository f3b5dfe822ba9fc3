"""Arguments kern::SparseCoalesce refuses with ValueError before any GPU call: no GPU exists
here, so a call that got past its checks would fail differently."""
import pytest

import ps_lite_amd as ps

_WS = ps._core.sparse_coalesce_workspace_bytes
# a valid call but for the GPU: ids, n, key_shift, grad, grad_rows, row_len, keys, sums, inverse
_GOOD = dict(ids=64, n=8, key_shift=0, grad=256, grad_rows=8, row_len=4, uniq_keys=512, sums=1024,
             inverse=2048, workspace=4096, workspace_bytes=_WS(8))


@pytest.mark.parametrize("bad", [
    dict(n=1 << 31, workspace_bytes=1 << 62), dict(grad_rows=9), dict(row_len=0),
    dict(workspace_bytes=_WS(8) - 1), dict(key_shift=-1), dict(key_shift=64),
    dict(ids=68), dict(uniq_keys=516), dict(inverse=2052)])
def test_coalesce_rejects(bad):
    with pytest.raises(ValueError):
        ps._core.k_sparse_coalesce(**dict(_GOOD, **bad))


def test_coalesce_empty_and_workspace_size():
    assert ps._core.k_sparse_coalesce(**dict(_GOOD, n=0, grad_rows=0)) == 0  # no HIP call
    sizes = [_WS(n) for n in (0, 1, 2, 65, ps._core.coalesce_tile, ps._core.coalesce_tile + 1,
                              1 << 20, (1 << 31) - 1)]
    assert sizes == sorted(sizes) and sizes[0] > 0
