"""GpuSparseHandler with wire_dtype="bf16": pushed values and pulled rows are bf16 bits, a row
row_len / 2 of the floats lens counts. cmd=1 assigns the bits, a pull returns the table's bits
(sparse_table_ptr()), cmd=0 is one step within test_sparse_bf16.py's rule from the table and
state as they lay before it, cmd=2 adds; a checkpoint loads under the fp32 wire."""
import threading

import numpy as np
import pytest

import ps_lite_amd as ps
from test_handler_paths import _Buf, _Node, _i32, _u64
from test_sparse_adagrad_handler import _message
from test_sparse_bf16 import _bf16, _widen, step_reference, stored_ok
from test_sparse_bf16_handler import _ROWS, _U, _handle, _lies
from test_sparse_lazy_adam import fresh


@pytest.mark.gpu
@pytest.mark.parametrize("row_len", [2, 64])
@pytest.mark.parametrize("optimizer", ["rowwise_adagrad", "lazy_adam"])
def test_bf16_wire_handler(optimizer, row_len, tmp_path):
    rng = np.random.default_rng([row_len, len(optimizer)])
    opt, rowwise = optimizer.replace("rowwise_", ""), optimizer.startswith("rowwise")
    nstate = _ROWS if opt == "adagrad" else fresh(_ROWS, row_len, rowwise).size
    with _Node("sparse") as node:
        _handle(node.server, optimizer, row_len, seed=5, wire_dtype="bf16")
        w, every = node.worker, _u64(range(_ROWS))

        def pull(keys, wire=np.uint16):
            per = row_len * np.dtype(wire).itemsize
            dst = _Buf(ps, len(keys) * per)
            w.wait(w.zpull_ptr(keys, dst.ptr, dst.n, 0, _i32([per // 4] * len(keys))))
            return dst.read()[dst.lead:dst.lead + dst.n].view(wire).reshape(-1, row_len)

        def push(keys, bits, cmd, fused=False):  # -> the bits a pull returns
            lens = _i32([row_len // 2] * len(keys))
            src, dst = _Buf(ps, bits.reshape(-1).view(np.uint8)), _Buf(ps, bits.size * 2)
            if not fused:
                w.wait(w.zpush_ptr(keys, src.ptr, src.n, 0, lens, cmd=cmd))
                return pull(keys)
            w.wait(w.zpushpull_ptr(keys, src.ptr, dst.ptr, src.n, 0, lens, cmd=cmd))
            return dst.read()[dst.lead:dst.lead + dst.n].view(np.uint16).reshape(-1, row_len)

        def lies():
            bits, st = _lies(ps, node.server, row_len, nstate)
            return bits, st.reshape(-1) if opt == "adagrad" else st

        init = _bf16(rng.standard_normal((_ROWS, row_len)))
        assert np.array_equal(push(every, init, cmd=1), init) and np.array_equal(lies()[0], init)
        for fused in (True, False):  # one step each way
            keys, local, grads = _message(rng, row_len)
            inside, rows, gbits = local >= 0, local[local >= 0], _bf16(grads)
            bits, state = lies()
            got = push(keys, gbits, cmd=0, fused=fused)
            w_ref, w_bound, st_ref, st_bound = step_reference(
                opt, rowwise, _widen(bits[rows]), state[rows], _widen(gbits[inside]).astype(np.float64))
            assert stored_ok(_widen(got[inside]), w_ref, w_bound, "stochastic") and not got[~inside].any()
            after = lies()
            assert np.all(np.abs(after[1][rows] - st_ref) <= st_bound)
            bits[rows], state[rows] = got[inside], after[1][rows]  # the response is the table's bits
            assert np.array_equal(after[0], bits) and np.array_equal(after[1], state)
        # cmd=2: one fp32 add, then R; the state stays. Values near 8 keep a sum of two bf16 off
        # exact zero, where the rule's ulp is zero
        keys, local, vals = _message(rng, row_len)
        inside, rows, vbits = local >= 0, local[local >= 0], _bf16(8 + vals)
        got = push(keys, vbits, cmd=2)
        total = _widen(bits[rows]).astype(np.float64) + _widen(vbits[inside])
        assert stored_ok(_widen(got[inside]), total, _U * np.abs(total), "stochastic")
        assert np.array_equal(lies()[1], state) and np.array_equal(lies()[0][rows], got[inside])
        # the wire dtype is not in a checkpoint: the fp32 wire pulls the same rows widened
        path, pulled = str(tmp_path / "wire.ckpt"), pull(every)
        node.server.save_checkpoint(path)
        _handle(node.server, optimizer, row_len, seed=5)
        node.server.load_checkpoint(path)
        assert np.array_equal(pull(every, np.float32).view(np.uint32), _widen(pulled).view(np.uint32))


def test_sparse_handle_rejects_bad_wire_dtype():
    """ValueError before any GPU call: no GPU and no HBM pool exist here"""
    roles = ("scheduler", "server", "worker")
    ps.setup_env(1, 1, root_port=30985)
    ths = [threading.Thread(target=ps.start, kwargs=dict(role=r, device=-1)) for r in roles]
    [t.start() for t in ths]
    [t.join() for t in ths]
    try:
        server = ps.KVServer(0)
        for row_len, bad in [(8, dict(wire_dtype="fp16", table_dtype="bf16")), (8, dict(wire_dtype="bf16")),
                             (7, dict(wire_dtype="bf16", table_dtype="bf16"))]:
            with pytest.raises(ValueError):
                server.set_gpu_sparse_handle(64, row_len, optimizer="adagrad", **bad)
        server.set_default_handle()
    finally:
        ths = [threading.Thread(target=ps.finalize, kwargs=dict(role=r)) for r in roles]
        [t.start() for t in ths]
        [t.join() for t in ths]
        ps.clear_registry()
