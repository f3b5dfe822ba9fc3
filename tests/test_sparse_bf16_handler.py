"""GpuSparseHandler over a bf16 table: the wire stays fp32, cmd=1 assigns RNE_bf16, cmd=0 is one
step within test_sparse_bf16.py's rule for a stored value, from the table (sparse_table_ptr(),
uint16) and the state (sparse_state_ptr()) as they lay before it, cmd=2 adds; a checkpoint
carries the launch counter, so a restored handler rounds the next message the same way."""
import numpy as np
import pytest

import ps_lite_amd as ps
from test_handler_paths import _HALF, _Buf, _Node, _i32, _two_procs, _u64
from test_sparse_adagrad_handler import _message, _pulled
from test_sparse_bf16 import _bf16, _widen, step_reference, stored_ok
from test_sparse_lazy_adam import _B1, _B2, _EPS, _LR, fresh

pytestmark = pytest.mark.gpu

_ROWS, _SHIFT, _U = 64, 48, 2.0 ** -23


def _handle(server, optimizer, row_len, **kw):
    betas = dict(beta1=_B1, beta2=_B2) if "adam" in optimizer else {}
    server.set_gpu_sparse_handle(_ROWS, row_len, optimizer=optimizer, lr=_LR, eps=_EPS,
                                 table_dtype="bf16", **betas, **kw)


def _lies(mod, server, row_len, state_floats):
    """(the table's bf16 bits, the state) as they lie on the server"""
    tab, st = _Buf(mod, _ROWS * row_len * 2), _Buf(mod, state_floats * 4)
    mod._core.k_dense_assign(tab.ptr, server.sparse_table_ptr(), tab.n)
    mod._core.k_dense_assign(st.ptr, server.sparse_state_ptr(), st.n)
    bits = tab.read()[tab.lead:tab.lead + tab.n].view(np.uint16).reshape(_ROWS, row_len)
    return bits, _pulled(st, 1).reshape(_ROWS, -1)


@pytest.mark.parametrize("row_len", [3, 64])
@pytest.mark.parametrize("optimizer", ["rowwise_adagrad", "lazy_adam"])
def test_bf16_handler_steps_and_checkpoint(optimizer, row_len, tmp_path):
    rng = np.random.default_rng([row_len, len(optimizer)])
    opt, rowwise = optimizer.replace("rowwise_", ""), optimizer.startswith("rowwise")
    nstate = _ROWS if opt == "adagrad" else fresh(_ROWS, row_len, rowwise).size
    with _Node("sparse") as node:
        _handle(node.server, optimizer, row_len, seed=5)
        w, every = node.worker, _u64(range(_ROWS))

        def push(keys, vals, cmd, fused=False):  # -> the rows a pull returns
            lens = _i32([row_len] * len(keys))
            src, dst = _Buf(ps, vals.reshape(-1).view(np.uint8)), _Buf(ps, vals.size * 4)
            if fused:
                w.wait(w.zpushpull_ptr(keys, src.ptr, dst.ptr, src.n, 0, lens, cmd=cmd))
            else:
                w.wait(w.zpush_ptr(keys, src.ptr, src.n, 0, lens, cmd=cmd))
                w.wait(w.zpull_ptr(keys, dst.ptr, dst.n, 0, lens))
            return _pulled(dst, row_len)

        def lies():
            bits, st = _lies(ps, node.server, row_len, nstate)
            return bits, st.reshape(-1) if opt == "adagrad" else st

        init = rng.standard_normal((_ROWS, row_len)).astype(np.float32)
        got = push(every, init, cmd=1)
        assert np.array_equal(got.view(np.uint32), _widen(_bf16(init)).view(np.uint32))
        assert np.array_equal(lies()[0], _bf16(init))
        for fused in (True, False):  # one step each way
            keys, local, grads = _message(rng, row_len)
            inside, rows = local >= 0, local[local >= 0]
            bits, state = lies()
            got = push(keys, grads, cmd=0, fused=fused)
            w_ref, w_bound, st_ref, st_bound = step_reference(
                opt, rowwise, _widen(bits[rows]), state[rows], grads[inside].astype(np.float64))
            assert stored_ok(got[inside], w_ref, w_bound, "stochastic") and not got[~inside].any()
            after = lies()
            assert np.all(np.abs(after[1][rows] - st_ref) <= st_bound)
            bits[rows], state[rows] = _bf16(got[inside]), after[1][rows]  # nothing else moved
            assert np.array_equal(after[0], bits) and np.array_equal(after[1], state)
            assert np.array_equal(_widen(bits[rows]), got[inside])  # the pull is the stored bf16
        # cmd=2: one fp32 add, then R; the state stays
        keys, local, vals = _message(rng, row_len)
        inside, rows = local >= 0, local[local >= 0]
        bits, state = lies()
        got = push(keys, vals, cmd=2)
        total = _widen(bits[rows]).astype(np.float64) + vals[inside]
        assert stored_ok(got[inside], total, _U * np.abs(total), "stochastic")
        saved = lies()
        assert np.array_equal(saved[1], state) and np.array_equal(_widen(saved[0][rows]), got[inside])
        # a fresh handler from the checkpoint rounds the next message as this one does
        path = str(tmp_path / "bf16.ckpt")
        node.server.save_checkpoint(path)
        keys, local, grads = _message(rng, row_len)
        first = push(keys, grads, cmd=0, fused=True), *lies()
        assert not np.array_equal(first[1], saved[0])
        _handle(node.server, optimizer, row_len, seed=5)
        node.server.load_checkpoint(path)
        assert all(np.array_equal(x, y) for x, y in zip(lies(), saved))
        again = push(keys, grads, cmd=0, fused=True), *lies()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))


def _two_workers_fn(ps_mod, rank):
    """test_sparse_lazy_adam_handler.py's two workers on a bf16 table under nearest: each shard
    holds one of the two serial orders. The first step's stored value lies within half an ulp
    plus its bound of the reference, which the second step's bound carries."""
    server, row_len = ps_mod.KVServer(0), 64
    _handle(server, "rowwise_lazy_adam", row_len, key_shift=_SHIFT, rounding="nearest")
    ps_mod.barrier("worker", ps_mod.WORKER_GROUP)  # both tables are up
    worker = ps_mod.KVWorker(0, 0)
    local = np.array(sorted(np.random.default_rng(31).choice(_ROWS, size=33, replace=False).tolist())
                     + [-1])
    n = len(local)
    shard = [b + (int(r) if r >= 0 else _ROWS) for b in (0, _HALF >> _SHIFT) for r in local]
    keys = _u64([r << _SHIFT for r in shard])  # sorted: rows ascend
    grads = [np.random.default_rng([32, r]).standard_normal((2 * n, row_len)).astype(np.float32)
             for r in (0, 1)]
    lens = _i32([row_len] * len(keys))
    src, dst = _Buf(ps_mod, grads[rank].reshape(-1).view(np.uint8)), _Buf(ps_mod, 8 * n * row_len)
    worker.wait(worker.zpush_ptr(keys, src.ptr, src.n, 0, lens, cmd=0))
    ps_mod.barrier("worker", ps_mod.WORKER_GROUP)  # both steps are in
    worker.wait(worker.zpull_ptr(keys, dst.ptr, dst.n, 0, lens))
    got = _pulled(dst, row_len)
    for sh in (0, 1):
        fits = []
        for order in ((0, 1), (1, 0)):
            g = [grads[r][sh * n:(sh + 1) * n - 1].astype(np.float64) for r in order]
            w1, b1, st1, sb1 = step_reference("lazy_adam", True, np.zeros((n - 1, row_len)),
                                              fresh(n - 1, row_len, True), g[0])
            half_ulp = 2.0 ** (np.floor(np.log2(np.abs(w1) + b1)) - 8)
            w2, b2, _, _ = step_reference("lazy_adam", True, w1, st1, g[1], bw=b1 + half_ulp, sb=sb1)
            fits.append(stored_ok(got[sh * n:(sh + 1) * n - 1], w2, b2, "nearest")
                        and not got[(sh + 1) * n - 1].any())
        assert any(fits), "shard %d matches neither serial order" % sh
    ps_mod.barrier("worker", ps_mod.WORKER_GROUP)  # nobody still uses this table
    return "ok", server


def test_two_workers_bf16_steps_are_atomic():
    _two_procs(_two_workers_fn)
