"""GpuSparseHandler over a bf16 table against tests/bf16_store_model.py, bit for bit: the n-th
launch that rounds (steps and adds, from 0; assigns and pulls count for nothing) rounds with
launch_seed(seed, n), keyed on the local table row behind key_shift, and a checkpoint carries n.
The table is read through sparse_table_ptr(), the state through sparse_state_ptr(). An add is one
fp32 add, so numpy's float32 sum is the kernel's x; the closing Adagrad step runs on gradients
k / 16 (test_sparse_bf16_exact.py: no contraction changes such a step). The 16-bit wire needs an
even row length, so it runs at 64 alone."""
import numpy as np
import pytest

import bf16_store_model as model
import ps_lite_amd as ps
from test_handler_paths import _Buf, _Node, _i32, _u64
from test_sparse_bf16_handler import _ROWS, _handle, _lies
from test_sparse_lazy_adam import _EPS, _LR

pytestmark = pytest.mark.gpu

_SHIFT, _SEED, _ACC = 48, 5, 0.3


def _message(rng, row_len):
    """(keys, local rows or -1, fp32 values): 37 unique rows of the table behind key_shift with
    arbitrary low bits, three keys outside it, in any order"""
    local = np.array([int(r) for r in rng.choice(_ROWS, size=37, replace=False)] + [-1] * 3)
    keys = [(int(r) << _SHIFT) | int(rng.integers(0, 1 << _SHIFT)) for r in local[:37]]
    keys = _u64(keys + [_ROWS << _SHIFT, (_ROWS + 3) << _SHIFT, 2 ** 64 - 1])
    order = rng.permutation(40)
    return keys[order], local[order], rng.standard_normal((40, row_len)).astype(np.float32)


@pytest.mark.parametrize("row_len,wire", [(3, "f32"), (64, "f32"), (64, "bf16")])
def test_handler_rounds_launch_n_with_launch_seed_n(row_len, wire, tmp_path):
    rng = np.random.default_rng([row_len, len(wire)])
    w16 = wire == "bf16"
    per = row_len // 2 if w16 else row_len  # floats of a row on the wire

    def on_wire(x):  # fp32 values (bf16 ones on the 16-bit wire) as they travel
        u = np.ascontiguousarray(x).view(np.uint32)
        assert not (w16 and (u & 0xFFFF).any())
        return (u >> 16).astype(np.uint16) if w16 else u

    def quantized(x):  # what a worker on this wire can push: any fp32, or a bf16
        return model.widen(model.store(x)) if w16 else x

    with _Node("sparse") as node:
        def handle():
            _handle(node.server, "adagrad", row_len, seed=_SEED, key_shift=_SHIFT, init_acc=_ACC,
                    **(dict(wire_dtype="bf16") if w16 else {}))

        handle()
        w = node.worker

        def pull(keys):  # -> the rows as they travel
            dst = _Buf(ps, len(keys) * per * 4)
            w.wait(w.zpull_ptr(keys, dst.ptr, dst.n, 0, _i32([per] * len(keys))))
            got = dst.read()[dst.lead:dst.lead + dst.n]
            return got.view(np.uint16 if w16 else np.uint32).reshape(len(keys), row_len)

        def push(keys, vals, cmd, fused=False):  # -> the rows a pull returns, as they travel
            lens = _i32([per] * len(keys))
            src, dst = _Buf(ps, on_wire(vals).reshape(-1).view(np.uint8)), _Buf(ps, len(keys) * per * 4)
            if not fused:
                w.wait(w.zpush_ptr(keys, src.ptr, src.n, 0, lens, cmd=cmd))
                src.check_unchanged("push")
                return pull(keys)
            w.wait(w.zpushpull_ptr(keys, src.ptr, dst.ptr, src.n, 0, lens, cmd=cmd))
            got = dst.read()[dst.lead:dst.lead + dst.n]
            return got.view(np.uint16 if w16 else np.uint32).reshape(len(keys), row_len)

        def lies():
            return _lies(ps, node.server, row_len, _ROWS * row_len)

        def travels(tab, local):  # the table's rows of a message as a pull returns them
            rows = np.where((local >= 0)[:, None], tab[np.maximum(local, 0)], 0).astype(np.uint16)
            return rows if w16 else rows.astype(np.uint32) << 16

        def add(tab, n, msg=None):  # one cmd=2 message as the model's n-th launch; -> (table, message)
            keys, local, vals = msg = msg or _message(rng, row_len)
            vals = quantized(vals)
            inside, rows = local >= 0, local[local >= 0]
            want = tab.copy()
            want[rows] = model.store(model.widen(tab[rows]) + vals[inside],
                                     model.r16(model.launch_seed(_SEED, n), rows, row_len))
            got = push(keys, vals, cmd=2)
            after, state = lies()
            assert np.array_equal(after, want), "add rounded with another seed than launch %d's" % n
            assert np.array_equal(got, travels(want, local))
            assert np.array_equal(state.view(np.uint32), state0.view(np.uint32))  # an add keeps the state
            if n:  # the counter matters: launch 0's seed leaves other bits
                stale = model.store(model.widen(tab[rows]) + vals[inside], model.r16(
                    model.launch_seed(_SEED, 0), rows, row_len))
                assert not np.array_equal(stale, want[rows])
            return want, msg

        every = _u64([r << _SHIFT for r in range(_ROWS)])
        init = quantized(rng.standard_normal((_ROWS, row_len)).astype(np.float32))
        tab = model.store(init)  # cmd=1 rounds to nearest even and counts for nothing
        assert np.array_equal(push(every, init, cmd=1), travels(tab, np.arange(_ROWS)))
        got, state0 = lies()
        assert np.array_equal(got, tab) and np.all(state0 == np.float32(_ACC))
        tab, _ = add(tab, 0)
        assert np.array_equal(pull(every), travels(tab, np.arange(_ROWS)))
        tab, _ = add(tab, 1)
        path = str(tmp_path / "exact.ckpt")
        node.server.save_checkpoint(path)
        saved = tab
        tab, third = add(saved, 2)
        # a fresh handler from the checkpoint goes on at n = 2, not at 0
        handle()
        node.server.load_checkpoint(path)
        assert np.array_equal(lies()[0], saved)
        again, _ = add(saved, 2, third)
        assert np.array_equal(again, tab)
        # launch 3: one element-wise Adagrad step, push and pull fused
        keys, local, _ = _message(rng, row_len)
        inside, rows = local >= 0, local[local >= 0]
        grads = (rng.integers(-64, 65, (40, row_len)) / 16).astype(np.float32)
        grads[np.flatnonzero(inside)[0]] = 0.0  # a zero gradient keeps the weight's bits
        x, st = model.adagrad_step(model.widen(tab[rows]), state0[rows], grads[inside], _LR, _EPS, False)
        want, want_state = tab.copy(), state0.copy()
        want[rows], want_state[rows] = model.store(
            x, model.r16(model.launch_seed(_SEED, 3), rows, row_len)), st
        got = push(keys, grads, cmd=0, fused=True)
        after, state = lies()
        assert np.array_equal(after, want)
        assert np.array_equal(state.view(np.uint32), want_state.view(np.uint32))
        assert np.array_equal(got, travels(want, local))
        assert np.array_equal(after[local[np.flatnonzero(inside)[0]]], tab[local[np.flatnonzero(inside)[0]]])
