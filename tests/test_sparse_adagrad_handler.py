"""GpuSparseHandler with an optimizer against a float64 model of its store rule: cmd=0 is a
gradient step, cmd=1 assigns rows, the state changes on a step alone. Bounds are
test_sparse_adagrad.py's, accumulated per step: with u = 2^-23 a step adds (L + 3) * u * s to
the state's bound and u * (|w| + (L/2 + 5) * |step|) to the weight's, and the state error e
carried into a step moves it by |step| * e / (2 * s) to first order (d step / d s =
-step / (2 s)), which the weight's bound takes too. An assign sets a weight's bound to zero."""
import numpy as np
import pytest

import ps_lite_amd as ps
from test_handler_paths import _HALF, _Buf, _Node, _i32, _two_procs, _u64

pytestmark = pytest.mark.gpu

_U, _ROWS, _SHIFT = 2.0 ** -23, 64, 48
_EPS = float(np.float32(1e-6))
_LR = [float(np.float32(v)) for v in (0.05, 0.02)]


class _Model:
    def __init__(self, row_len, rowwise, init_acc):
        self.L, self.rowwise = row_len, rowwise
        self.w = np.zeros((_ROWS, row_len))
        self.s = np.full((_ROWS,) if rowwise else (_ROWS, row_len), float(init_acc))
        self.wb, self.sb = np.zeros_like(self.w), np.zeros_like(self.s)

    def assign(self, rows, vals):
        self.w[rows], self.wb[rows] = vals, 0.0

    def step(self, rows, g, lr):
        g = g.astype(np.float64)
        L = self.L if self.rowwise else 1
        s = self.s[rows] + ((g * g).sum(axis=1) / self.L if self.rowwise else g * g)
        carried = self.sb[rows]
        self.s[rows], self.sb[rows] = s, carried + (L + 3) * _U * s
        if self.rowwise:
            s, carried = s[:, None], carried[:, None]
        step = lr * g / (np.sqrt(s) + _EPS)
        with np.errstate(invalid="ignore", divide="ignore"):
            drift = np.where(step != 0, np.abs(step) * carried / (2 * s), 0.0)
        self.w[rows] -= step
        self.wb[rows] += _U * (np.abs(self.w[rows]) + (L / 2 + 5) * np.abs(step)) + drift

    def holds(self, local, got):
        """got: the pulled rows of the local rows (-1 = outside the table: zeros)"""
        inside = local >= 0
        err = np.abs(got[inside] - self.w[local[inside]])
        return not got[~inside].any() and bool((err <= self.wb[local[inside]]).all())


def _pulled(dst, row_len):
    return dst.read()[dst.lead:dst.lead + dst.n].view(np.float32).reshape(-1, row_len)


def _message(rng, row_len):
    """(keys, local rows or -1, gradients): unique rows, a zero gradient, keys outside"""
    local = np.array([int(r) for r in rng.choice(_ROWS, size=37, replace=False)] + [-1] * 3)
    keys = _u64(list(local[:37]) + [_ROWS, _ROWS + 3, 2 ** 64 - 1])
    order = rng.permutation(40)
    grads = rng.standard_normal((40, row_len)).astype(np.float32)
    grads[order.tolist().index(0)] = 0.0
    return keys[order], local[order], grads


@pytest.mark.parametrize("row_len", [3, 64])
@pytest.mark.parametrize("optimizer", ["adagrad", "rowwise_adagrad"])
def test_optimizer_steps_and_checkpoint(optimizer, row_len, tmp_path):
    rng = np.random.default_rng([row_len, len(optimizer)])
    with _Node("sparse") as node:
        node.server.set_gpu_sparse_handle(_ROWS, row_len, optimizer=optimizer, lr=_LR[0],
                                          eps=_EPS, init_acc=0.0)
        model = _Model(row_len, optimizer == "rowwise_adagrad", 0.0)
        w, every = node.worker, _u64(range(_ROWS))

        def push(keys, vals, cmd, fused=False, dev_keys=False):  # -> the rows a pull returns
            lens = _i32([row_len] * len(keys))
            kbuf = _Buf(ps, keys.view(np.uint8)) if dev_keys else None
            kptr = kbuf.ptr if dev_keys else 0
            src, dst = _Buf(ps, vals.reshape(-1).view(np.uint8)), _Buf(ps, vals.size * 4)
            if fused:
                w.wait(w.zpushpull_ptr(keys, src.ptr, dst.ptr, src.n, 0, lens, cmd=cmd,
                                       keys_dev_ptr=kptr))
            else:
                w.wait(w.zpush_ptr(keys, src.ptr, src.n, 0, lens, cmd=cmd, keys_dev_ptr=kptr))
                w.wait(w.zpull_ptr(keys, dst.ptr, dst.n, 0, lens, keys_dev_ptr=kptr))
            return _pulled(dst, row_len)

        def snapshot():  # (every row as pulled, the state) as bits
            dst, st = _Buf(ps, _ROWS * row_len * 4), _Buf(ps, model.s.size * 4)
            w.wait(w.zpull_ptr(every, dst.ptr, dst.n, 0, _i32([row_len] * _ROWS)))
            ps._core.k_dense_assign(st.ptr, node.server.sparse_state_ptr(), st.n)
            return _pulled(dst, row_len).view(np.uint32), _pulled(st, 1).view(np.uint32)

        init = rng.standard_normal((_ROWS, row_len)).astype(np.float32)
        assert np.array_equal(push(every, init, cmd=1).view(np.uint32), init.view(np.uint32))
        model.assign(np.arange(_ROWS), init)
        for i, lr in enumerate([_LR[0], _LR[1], _LR[1]]):
            if i == 1:
                node.server.set_sparse_lr(lr)
            keys, local, grads = _message(rng, row_len)
            got = push(keys, grads, cmd=0, fused=(i % 2 == 0), dev_keys=(i > 0))
            model.step(local[local >= 0], grads[local >= 0], lr)
            assert model.holds(local, got), "step %d" % i
        rows_saved, state_saved = snapshot()
        node.server.save_checkpoint(str(tmp_path / "adagrad.ckpt"))
        keys, local, grads = _message(rng, row_len)
        push(keys, grads, cmd=0, fused=True)
        rows_now, state_now = snapshot()
        assert not np.array_equal(rows_now, rows_saved) and not np.array_equal(state_now, state_saved)
        node.server.load_checkpoint(str(tmp_path / "adagrad.ckpt"))
        rows_now, state_now = snapshot()
        assert np.array_equal(rows_now, rows_saved) and np.array_equal(state_now, state_saved)


def _two_workers_fn(ps_mod, rank):
    """Both workers push one step to the same rows of both servers (zero weights, state
    0.25), meet at a barrier and pull: each server's shard holds one of the two serial
    orders. A lost or torn update matches neither."""
    server, worker = ps_mod.KVServer(0), None
    for optimizer, row_len in (("adagrad", 3), ("rowwise_adagrad", 64)):
        server.set_gpu_sparse_handle(_ROWS, row_len, key_shift=_SHIFT, optimizer=optimizer,
                                     lr=_LR[0], eps=_EPS, init_acc=0.25)
        ps_mod.barrier("worker", ps_mod.WORKER_GROUP)  # both tables are up
        worker = worker or ps_mod.KVWorker(0, 0)
        local = np.array(sorted(np.random.default_rng([31, row_len]).choice(
            _ROWS, size=33, replace=False).tolist()) + [-1])
        n = len(local)
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
        for sh in (0, 1):
            fits = []
            for order in ((0, 1), (1, 0)):
                model = _Model(row_len, optimizer == "rowwise_adagrad", 0.25)
                for r in order:
                    model.step(local[:-1], grads[r][sh * n:(sh + 1) * n - 1], _LR[0])
                fits.append(model.holds(local, got[sh * n:(sh + 1) * n]))
            assert any(fits), "%s shard %d matches neither serial order" % (optimizer, sh)
        ps_mod.barrier("worker", ps_mod.WORKER_GROUP)  # nobody still uses this table
    return "ok", server


def test_two_workers_steps_are_atomic():
    _two_procs(_two_workers_fn)
