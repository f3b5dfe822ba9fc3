"""Fused dense push+pull: the dual-write kernel (store entry + pull
destination from one read of the pushed values), the server fast path
and the worker's one-sided variant, plus every fallback to the two-kernel
sequence. All marked gpu."""
import threading

import numpy as np
import pytest

import ps_lite_amd as ps
from ps_lite_amd.parallel import launch_local

pytestmark = pytest.mark.gpu

_PORT = [28300]
_N = 4099  # floats per key: 16396 bytes, a non-empty 12-byte tail
_HALF = (1 << 64) // 2


def _boot_joint_inproc():
    _PORT[0] += 7
    ps.setup_env(1, 1, root_port=_PORT[0], XPS_DEV_ID=0, XPS_POOL_GB=4)
    ths = [threading.Thread(target=ps.start, kwargs=dict(role="scheduler", device=-1)),
           threading.Thread(target=ps.start, kwargs=dict(role="joint", device=0))]
    [t.start() for t in ths]
    [t.join() for t in ths]


def _down_joint():
    ths = [threading.Thread(target=ps.finalize, kwargs=dict(role="scheduler")),
           threading.Thread(target=ps.finalize, kwargs=dict(role="joint"))]
    [t.start() for t in ths]
    [t.join() for t in ths]
    ps.clear_registry()


# ------------------------------------------------------------------ kernel

_GUARD = 0xAB
_KERNEL_CASES = [
    (0, 0),
    (7, 0),
    (16, 0),
    (16 * (256 * 3 + 5) + 9, 0),
    ((1 << 20) + 3, 0),
    ((1 << 20) + 3, 8),  # capped grid: the stride loop runs ~32 iterations
]


def _run_assign2(nbytes, grid_cap, lead):
    """dst ranges start `lead` bytes into guard-filled buffers; returns
    (src, buf0, buf1) on the host after the kernel ran."""
    import torch

    g = torch.Generator(device="cpu").manual_seed(nbytes + grid_cap)
    src = torch.randint(0, 256, (max(nbytes, 1),), dtype=torch.uint8, generator=g)[:nbytes]
    src_d = src.to("cuda:0")
    bufs = [torch.full((lead + nbytes + 48,), _GUARD, dtype=torch.uint8, device="cuda:0")
            for _ in range(2)]
    ps._core.k_dense_assign2(bufs[0].data_ptr() + lead, bufs[1].data_ptr() + lead,
                             src_d.data_ptr(), nbytes, grid_cap)
    return src, bufs[0].cpu(), bufs[1].cpu()


@pytest.mark.parametrize("nbytes,grid_cap", _KERNEL_CASES)
def test_kernel_dense_assign2_vs_torch(nbytes, grid_cap):
    import torch

    lead = 16  # keeps the destinations 16 B-aligned: the vector path runs
    src, b0, b1 = _run_assign2(nbytes, grid_cap, lead)
    for b in (b0, b1):
        assert torch.equal(b[lead:lead + nbytes], src)
        assert bool((b[:lead] == _GUARD).all()) and bool((b[lead + nbytes:] == _GUARD).all())


def test_kernel_dense_assign2_misaligned_destinations():
    """Destinations off the 16 B grid take the byte loop for the whole
    range — same result, guards intact."""
    import torch

    nbytes, lead = 16 * 300 + 5, 4
    src, b0, b1 = _run_assign2(nbytes, 0, lead)
    for b in (b0, b1):
        assert torch.equal(b[lead:lead + nbytes], src)
        assert bool((b[:lead] == _GUARD).all()) and bool((b[lead + nbytes:] == _GUARD).all())


# ------------------------------------------------- in-process joint rounds

def _payload(step, nk, n):
    # distinct per step, per key and per element
    return [(np.arange(n, dtype=np.float32) * 0.5 + 1000.0 * step + 10.0 * i) for i in range(nk)]


def _fused_rounds(ps_mod, worker, steps=4):
    """3 keys x 4099 floats through round_mixed(overlap=True); returns the
    fused-launch counter delta of every step after checking the values."""
    nk, n = 3, _N
    keys = np.array([310, 311, 312], dtype=np.uint64)
    push = [ps_mod.pool_alloc(n * 4) for _ in range(nk)]
    pull = [ps_mod.pool_alloc(n * 4) for _ in range(nk)]
    third = ps_mod.pool_alloc(n * 4)
    lens = np.array([n], dtype=np.int32)
    deltas = []
    for step in range(steps):
        vals = _payload(step, nk, n)
        for b, v in zip(push, vals):
            b.copy_from(v)
        before = ps_mod._core.fused_assign_count()
        worker.round_mixed(keys, [b.ptr for b in push], [b.ptr for b in pull], [n * 4] * nk,
                           0, 1, True)
        deltas.append(ps_mod._core.fused_assign_count() - before)
        for i in range(nk):
            assert np.array_equal(pull[i].to_numpy_f32(), vals[i]), (step, i)
            # a plain pull proves the STORE was written, not only the dst
            worker.wait(worker.zpull_ptr(keys[i:i + 1], third.ptr, n * 4, 0, lens, cmd=1))
            assert np.array_equal(third.to_numpy_f32(), vals[i]), (step, i)
    return deltas


def test_fused_round_mixed_inproc():
    _boot_joint_inproc()
    try:
        server = ps.KVServer(0)
        server.set_gpu_dense_handle(mode="assign")
        worker = ps.KVWorker(0, 0)
        # step 1 learns the entry adverts with the plain pair; every later
        # step is exactly one dual-write launch per key
        assert _fused_rounds(ps, worker) == [0, 3, 3, 3]
    finally:
        _down_joint()


def _unfused_worker_fn(ps_mod, rank):
    server = ps_mod.KVServer(0)
    server.set_gpu_dense_handle(mode="assign")
    worker = ps_mod.KVWorker(0, 0)
    deltas = _fused_rounds(ps_mod, worker)
    return (deltas, int(ps_mod._core.fused_assign_count())), server


def test_fused_switch_off_in_child():
    """XPS_FUSED_ASSIGN=0: identical values (checked in the child), no
    dual-write launch at all."""
    results = launch_local(1, 1, _unfused_worker_fn, joint=True, devices={0: 0},
                           env_extra={"XPS_POOL_GB": 4, "XPS_FUSED_ASSIGN": 0}, timeout=300)
    deltas, total = results[0]
    assert deltas == [0, 0, 0, 0] and total == 0


def _local_one_sided_worker_fn(ps_mod, rank):
    server = ps_mod.KVServer(0)
    server.set_gpu_dense_handle(mode="assign")
    worker = ps_mod.KVWorker(0, 0)
    deltas = _fused_rounds(ps_mod, worker)
    # plain one-sided push, then pull, of a tiny and of a larger key
    for key, n in ((320, 3), (321, 1024)):
        keys = np.array([key], dtype=np.uint64)
        lens = np.array([n], dtype=np.int32)
        src, dst = ps_mod.pool_alloc(n * 4), ps_mod.pool_alloc(n * 4)
        for rep in range(2):  # the second push of a key is the one-sided one
            vals = np.arange(n, dtype=np.float32) * 0.75 - 5.0 + 100.0 * rep
            src.copy_from(vals)
            worker.wait(worker.zpush_ptr(keys, src.ptr, n * 4, 0, lens, cmd=1))
            worker.wait(worker.zpull_ptr(keys, dst.ptr, n * 4, 0, lens, cmd=1))
            assert np.array_equal(dst.to_numpy_f32(), vals), (key, rep)
    return deltas, server


def test_fused_local_one_sided_in_child():
    """XPS_LOCAL_ONE_SIDED=1: the worker's own write to a same-process
    server runs on the receiver plane's stream; identical values (checked
    in the child), one dual-write launch per key once the adverts are in."""
    results = launch_local(1, 1, _local_one_sided_worker_fn, joint=True, devices={0: 0},
                           env_extra={"XPS_POOL_GB": 4, "XPS_LOCAL_ONE_SIDED": 1}, timeout=300)
    assert results[0] == [0, 3, 3, 3]


# --------------------------------------------------------------- fallbacks

def test_fused_fallbacks_assign_handler():
    _boot_joint_inproc()
    try:
        server = ps.KVServer(0)
        server.set_gpu_dense_handle(mode="assign")
        worker = ps.KVWorker(0, 0)
        n = _N
        key = np.array([420], dtype=np.uint64)
        src, dst = ps.pool_alloc(n * 4), ps.pool_alloc(n * 4)
        count = ps._core.fused_assign_count

        def round_(s, d, nf, cmd):
            before = count()
            worker.round_mixed(key, [s.ptr], [d.ptr], [nf * 4], 0, cmd, True)
            return count() - before

        a = np.arange(n, dtype=np.float32) + 1.0
        b = np.arange(n, dtype=np.float32) * 0.25 - 3.0
        src.copy_from(a)
        assert round_(src, dst, n, 1) == 0  # learns the advert
        assert round_(src, dst, n, 1) == 1  # fused from now on
        assert np.array_equal(dst.to_numpy_f32(), a)

        # cmd=2 (sum): needs the accumulate kernel, never fused
        src.copy_from(b)
        assert round_(src, dst, n, 2) == 0
        assert np.array_equal(dst.to_numpy_f32(), a + b)

        # re-push at another length: the advert no longer matches, the
        # plain pair re-learns it, the step after that fuses again
        m = 2 * n + 1
        src2, dst2 = ps.pool_alloc(m * 4), ps.pool_alloc(m * 4)
        c = np.arange(m, dtype=np.float32) * 2.0 + 7.0
        src2.copy_from(c)
        assert round_(src2, dst2, m, 1) == 0
        assert np.array_equal(dst2.to_numpy_f32(), c)
        src2.copy_from(c + 1.0)
        assert round_(src2, dst2, m, 1) == 1
        assert np.array_equal(dst2.to_numpy_f32(), c + 1.0)

        # fused request with HOST buffers: staged, two-step on the server
        hsrc, hdst = ps.host_alloc(m * 4), ps.host_alloc(m * 4)
        d = np.arange(m, dtype=np.float32) - 11.0
        hsrc.copy_from(d)
        before = count()
        worker.wait(worker.zpushpull_ptr(key, hsrc.ptr, hdst.ptr, m * 4, -1,
                                         np.array([m], dtype=np.int32), cmd=1))
        assert count() == before
        assert np.array_equal(hdst.to_numpy_f32(), d)
    finally:
        _down_joint()


def test_fused_never_on_reduce_handler():
    """A reduce-mode handler advertises no entries (and rejects fused
    requests): round_mixed keeps issuing the plain pair."""
    _boot_joint_inproc()
    try:
        server = ps.KVServer(0)
        server.set_gpu_dense_handle(mode="reduce")
        worker = ps.KVWorker(0, 0)
        nk, n = 2, _N
        keys = np.array([530, 531], dtype=np.uint64)
        push = [ps.pool_alloc(n * 4) for _ in range(nk)]
        pull = [ps.pool_alloc(n * 4) for _ in range(nk)]
        before = ps._core.fused_assign_count()
        for step in range(3):
            vals = _payload(step, nk, n)
            for buf, v in zip(push, vals):
                buf.copy_from(v)
            worker.round_mixed(keys, [x.ptr for x in push], [x.ptr for x in pull],
                               [n * 4] * nk, 0, 0, True)
            for i in range(nk):
                assert np.array_equal(pull[i].to_numpy_f32(), vals[i]), (step, i)
        assert ps._core.fused_assign_count() == before
    finally:
        _down_joint()


# ----------------------------------------------------------- cross-process

def _cross_worker_fn(ps_mod, rank):
    """Two joint processes on one GPU. Per-rank keys (single writer) on
    BOTH servers; the remote-owned key takes the worker's one-sided
    EntryPushPull from step 2 on."""
    server = ps_mod.KVServer(0)
    server.set_gpu_dense_handle(mode="assign")
    ps_mod.barrier("worker", ps_mod.WORKER_GROUP)
    worker = ps_mod.KVWorker(0, 0)
    n = _N
    own = {0: 100 + rank, 1: _HALF + 200 + rank}  # server rank -> our key there
    remote_key = np.array([own[1 - rank]], dtype=np.uint64)
    local_key = np.array([own[rank]], dtype=np.uint64)
    bufs = {name: (ps_mod.pool_alloc(n * 4), ps_mod.pool_alloc(n * 4))
            for name in ("remote", "local")}
    third = ps_mod.pool_alloc(n * 4)
    lens = np.array([n], dtype=np.int32)
    count = ps_mod._core.fused_assign_count
    remote_fused = 0
    for step in range(3):
        for name, key in (("remote", remote_key), ("local", local_key)):
            src, dst = bufs[name]
            vals = (np.arange(n, dtype=np.float32) + 100.0 * (rank + 1) + 10.0 * step +
                    (0.5 if name == "remote" else 0.0))
            src.copy_from(vals)
            before = count()
            worker.round_mixed(key, [src.ptr], [dst.ptr], [n * 4], 0, 1, True)
            if name == "remote":
                remote_fused += count() - before
            assert np.array_equal(dst.to_numpy_f32(), vals), (step, name)
            worker.wait(worker.zpull_ptr(key, third.ptr, n * 4, 0, lens, cmd=1))
            assert np.array_equal(third.to_numpy_f32(), vals), (step, name)
    ps_mod.barrier("worker", ps_mod.WORKER_GROUP)
    return int(remote_fused), server


def test_fused_cross_process_one_sided():
    results = launch_local(2, 2, _cross_worker_fn, joint=True, devices={0: 0, 1: 0},
                           env_extra={"XPS_POOL_GB": 4}, timeout=300)
    assert len(results) == 2
    for rank, remote_fused in results.items():
        assert remote_fused > 0, results
