"""GpuSparseHandler with a lazy-Adam optimizer: cmd=1 assigns rows and leaves the state fresh,
cmd=0 is one step, checked against test_sparse_lazy_adam.py's float64 reference and bound from
the table and the state records as they lay before it (read through sparse_state_ptr()), so
nothing drifts; the two-worker test carries the first step's bounds into the second."""
import numpy as np
import pytest

import ps_lite_amd as ps
from test_handler_paths import _HALF, _Buf, _Node, _i32, _two_procs, _u64
from test_sparse_adagrad_handler import _message, _pulled
from test_sparse_lazy_adam import _B1, _B2, _EPS, fresh, reference, worst

pytestmark = pytest.mark.gpu

_ROWS, _SHIFT = 64, 48
_LR = [float(np.float32(v)) for v in (0.05, 0.02)]
_OPT = dict(eps=_EPS, beta1=_B1, beta2=_B2)


def _state(mod, server, row_len, rowwise):
    """the server's state records, (_ROWS, record floats) fp32"""
    st = _Buf(mod, fresh(_ROWS, row_len, rowwise).size * 4)
    mod._core.k_dense_assign(st.ptr, server.sparse_state_ptr(), st.n)
    return _pulled(st, 1).reshape(_ROWS, -1)


def _same(a, b):  # bit for bit
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("row_len", [3, 64])
@pytest.mark.parametrize("optimizer", ["lazy_adam", "rowwise_lazy_adam"])
def test_lazy_adam_steps_and_checkpoint(optimizer, row_len, tmp_path):
    rng, rowwise = np.random.default_rng([row_len, len(optimizer)]), optimizer.startswith("rowwise")
    with _Node("sparse") as node:
        node.server.set_gpu_sparse_handle(_ROWS, row_len, optimizer=optimizer, lr=_LR[0], **_OPT)
        w, every = node.worker, _u64(range(_ROWS))

        def push(keys, vals, cmd, fused=False, dev_keys=False):  # -> the rows a pull returns
            lens, kbuf = _i32([row_len] * len(keys)), _Buf(ps, keys.view(np.uint8))
            kptr = kbuf.ptr if dev_keys else 0
            src, dst = _Buf(ps, vals.reshape(-1).view(np.uint8)), _Buf(ps, vals.size * 4)
            if fused:
                w.wait(w.zpushpull_ptr(keys, src.ptr, dst.ptr, src.n, 0, lens, cmd=cmd,
                                       keys_dev_ptr=kptr))
            else:
                w.wait(w.zpush_ptr(keys, src.ptr, src.n, 0, lens, cmd=cmd, keys_dev_ptr=kptr))
                w.wait(w.zpull_ptr(keys, dst.ptr, dst.n, 0, lens, keys_dev_ptr=kptr))
            return _pulled(dst, row_len)

        def snapshot():  # (every row as pulled, the state records)
            dst = _Buf(ps, _ROWS * row_len * 4)
            w.wait(w.zpull_ptr(every, dst.ptr, dst.n, 0, _i32([row_len] * _ROWS)))
            return _pulled(dst, row_len), _state(ps, node.server, row_len, rowwise)

        init = rng.standard_normal((_ROWS, row_len)).astype(np.float32)
        assert _same([push(every, init, cmd=1)], [init])
        assert _same(snapshot(), (init, fresh(_ROWS, row_len, rowwise)))
        for i, lr in enumerate([_LR[0], _LR[1], _LR[1]]):
            if i == 1:
                node.server.set_sparse_lr(lr)
            keys, local, grads = _message(rng, row_len)
            inside, rows = local >= 0, local[local >= 0]
            table, state = snapshot()
            got = push(keys, grads, cmd=0, fused=(i % 2 == 0), dev_keys=(i > 0))
            w_ref, w_bound, st_ref, st_bound = reference(table[rows], state[rows], grads[inside],
                                                         lr, rowwise)
            after = snapshot()
            assert worst(got[inside], w_ref, w_bound) <= 1.0 and not got[~inside].any(), i
            assert worst(after[1][rows], st_ref, st_bound) <= 1.0, i
            table[rows], state[rows] = got[inside], after[1][rows]  # nothing else moved
            assert _same(after, (table, state)), i
        saved = snapshot()
        node.server.save_checkpoint(str(tmp_path / "lazy_adam.ckpt"))
        keys, local, grads = _message(rng, row_len)
        push(keys, grads, cmd=0, fused=True)
        assert not any(_same([x], [y]) for x, y in zip(snapshot(), saved))
        node.server.load_checkpoint(str(tmp_path / "lazy_adam.ckpt"))
        assert _same(snapshot(), saved)


def _two_workers_fn(ps_mod, rank):
    """Both workers push one step to the same rows of both servers (zero weights, a fresh
    state), meet at a barrier and pull: each server's shard holds one of the two serial
    orders, and every stepped row has p1 = beta1 * beta1. A lost or torn update shows."""
    server, worker = ps_mod.KVServer(0), None
    for optimizer, row_len in (("lazy_adam", 3), ("rowwise_lazy_adam", 64)):
        rowwise = optimizer.startswith("rowwise")
        server.set_gpu_sparse_handle(_ROWS, row_len, key_shift=_SHIFT, optimizer=optimizer,
                                     lr=_LR[0], **_OPT)
        ps_mod.barrier("worker", ps_mod.WORKER_GROUP)  # both tables are up
        worker = worker or ps_mod.KVWorker(0, 0)
        local = np.array(sorted(np.random.default_rng([31, row_len]).choice(
            _ROWS, size=33, replace=False).tolist()) + [-1])
        n, rows = len(local), local[:-1]
        shard = [b + (int(r) if r >= 0 else _ROWS) for b in (0, _HALF >> _SHIFT) for r in local]
        keys = _u64([r << _SHIFT for r in shard])  # sorted: rows ascend
        grads = [np.random.default_rng([32, row_len, r]).standard_normal(
            (2 * n, row_len)).astype(np.float32) for r in (0, 1)]
        lens = _i32([row_len] * len(keys))
        src, dst = _Buf(ps_mod, grads[rank].reshape(-1).view(np.uint8)), _Buf(ps_mod, 8 * n * row_len)
        worker.wait(worker.zpush_ptr(keys, src.ptr, src.n, 0, lens, cmd=0))
        ps_mod.barrier("worker", ps_mod.WORKER_GROUP)  # both steps are in
        worker.wait(worker.zpull_ptr(keys, dst.ptr, dst.n, 0, lens))
        got = _pulled(dst, row_len)
        p1 = _state(ps_mod, server, row_len, rowwise)[:, 0]  # this process's own shard
        want = np.ones(_ROWS, dtype=np.float32)
        want[rows] = np.float32(_B1) * np.float32(_B1)
        assert _same([p1], [want])
        for sh in (0, 1):
            fits = []
            for order in ((0, 1), (1, 0)):
                s = (np.zeros((n - 1, row_len)), 0.0, fresh(n - 1, row_len, rowwise), None)
                for r in order:
                    s = reference(s[0], s[2], grads[r][sh * n:(sh + 1) * n - 1], _LR[0], rowwise,
                                  bw=s[1], sb=s[3])
                err = np.abs(got[sh * n:(sh + 1) * n - 1] - s[0])
                fits.append(bool((err <= s[1]).all()) and not got[(sh + 1) * n - 1].any())
            assert any(fits), "%s shard %d matches neither serial order" % (optimizer, sh)
        ps_mod.barrier("worker", ps_mod.WORKER_GROUP)  # nobody still uses this table
    return "ok", server


def test_two_workers_lazy_adam_steps_are_atomic():
    _two_procs(_two_workers_fn)
