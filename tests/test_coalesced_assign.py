"""Coalesced fused dense push+pull: the batched dual-write kernel and the
per-stream launch coalescer of the GPU plane (keys queued behind a busy
GPU share one launch and one event). All marked gpu."""
import os
import threading

import numpy as np
import pytest

import ps_lite_amd as ps
from ps_lite_amd.parallel import launch_local

pytestmark = pytest.mark.gpu

_PORT = [29100]
_N = 4096  # floats per key: 16 KiB, a whole number of 16 B chunks
_HALF = (1 << 64) // 2
_HOLD = "XPS_COALESCE_HOLD"


def _boot_joint_inproc(hold):
    _PORT[0] += 7
    ps.setup_env(1, 1, root_port=_PORT[0], XPS_DEV_ID=0, XPS_POOL_GB=4,
                 **{_HOLD: 1 if hold else 0})
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
    # the test-only switch must not linger for later clusters of this process
    ps.init_env({_HOLD: "0"})
    os.environ.pop(_HOLD, None)


# ------------------------------------------------------------------ kernel

_GUARD = 0xAB
_LEAD, _TRAIL = 16, 48  # guard bytes around every destination range
_MIXED = [16, 4096, 16 * (256 * 3 + 5), (1 << 20) + 16, 48]
_KERNEL_CASES = [
    ("one16", [16], 0),
    ("mixed", _MIXED, 0),
    ("split70", [4096] * 70, 0),  # more than kMaxBatch: two launches
    ("mixed_cap2", _MIXED, 2),    # two blocks: many tile iterations each
]


@pytest.mark.parametrize("name,sizes,tile_cap", _KERNEL_CASES,
                         ids=[c[0] for c in _KERNEL_CASES])
def test_kernel_batched_assign2_vs_torch(name, sizes, tile_cap):
    import torch

    g = torch.Generator(device="cpu").manual_seed(len(sizes) * 131 + tile_cap)
    total = sum(sizes)
    src = torch.randint(0, 256, (total,), dtype=torch.uint8, generator=g)
    src_d = src.to("cuda:0")
    span = sum(s + _LEAD + _TRAIL for s in sizes)
    expect = torch.full((span,), _GUARD, dtype=torch.uint8)
    bufs = [torch.full((span,), _GUARD, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    segs, s_at, d_at = [], 0, 0
    for n in sizes:
        d_at += _LEAD
        segs.append((bufs[0].data_ptr() + d_at, bufs[1].data_ptr() + d_at,
                     src_d.data_ptr() + s_at, n))
        expect[d_at:d_at + n] = src[s_at:s_at + n]
        d_at += n + _TRAIL
        s_at += n
    ps._core.k_batched_assign2(segs, tile_cap)
    # payload and every guard byte at once: a byte copy, no tolerance
    for b in bufs:
        assert torch.equal(b.cpu(), expect)
    assert torch.equal(src_d.cpu(), src)


# ------------------------------------------------- in-process joint rounds

def _payload(step, nk, n, salt=0.0):
    return [(np.arange(n, dtype=np.float32) * 0.5 + 1000.0 * step + 10.0 * i + salt)
            for i in range(nk)]


def _rounds(ps_mod, worker, keys, sizes, steps=3, salt=0.0):
    """round_mixed(overlap=True) over `keys` (`sizes` floats each); checks
    every pull and the store per step, returns ([(key delta, launch delta)
    per step], [pulled values per step])."""
    nk = len(keys)
    push = [ps_mod.pool_alloc(n * 4) for n in sizes]
    pull = [ps_mod.pool_alloc(n * 4) for n in sizes]
    third = ps_mod.pool_alloc(max(sizes) * 4)
    count, launches = ps_mod._core.fused_assign_count, ps_mod._core.fused_assign_launches
    deltas, seen = [], []
    for step in range(steps):
        vals = [_payload(step, nk, n, salt)[i] for i, n in enumerate(sizes)]
        for b, v in zip(push, vals):
            b.copy_from(v)
        c0, l0 = count(), launches()
        worker.round_mixed(keys, [b.ptr for b in push], [b.ptr for b in pull],
                           [n * 4 for n in sizes], 0, 1, True)
        deltas.append((count() - c0, launches() - l0))
        got = [pull[i].to_numpy_f32()[:sizes[i]].copy() for i in range(nk)]
        for i in range(nk):
            assert np.array_equal(got[i], vals[i]), (step, i)
            # a plain pull proves the STORE was written, not only the dst
            lens = np.array([sizes[i]], dtype=np.int32)
            worker.wait(worker.zpull_ptr(keys[i:i + 1], third.ptr, sizes[i] * 4, 0, lens, cmd=1))
            assert np.array_equal(third.to_numpy_f32()[:sizes[i]], vals[i]), (step, i)
        seen.append(got)
    return deltas, seen


def _joint_round_70(hold):
    _boot_joint_inproc(hold)
    try:
        server = ps.KVServer(0)
        server.set_gpu_dense_handle(mode="assign")
        worker = ps.KVWorker(0, 0)
        keys = np.arange(7000, 7070, dtype=np.uint64)
        out = _rounds(ps, worker, keys, [_N] * 70)
        del server
        return out
    finally:
        _down_joint()


def test_joint_round_hold_then_default():
    deltas, held = _joint_round_70(hold=True)
    assert deltas[0][0] == 0  # step 1 learns the entry adverts with the plain pair
    for kd, ld in deltas[1:]:
        # 64 keys fill a batch, the other 6 wait for the completion thread
        assert kd == 70 and 1 <= ld <= 3, deltas
    deltas, free = _joint_round_70(hold=False)
    for kd, ld in deltas[1:]:
        assert kd == 70 and 1 <= ld <= 70, deltas
    for a, b in zip(held, free):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_same_key_twice_in_one_burst():
    _boot_joint_inproc(hold=True)
    try:
        server = ps.KVServer(0)
        server.set_gpu_dense_handle(mode="assign")
        worker = ps.KVWorker(0, 0)
        n = _N
        key = np.array([7200], dtype=np.uint64)
        lens = np.array([n], dtype=np.int32)
        src = [ps.pool_alloc(n * 4) for _ in range(2)]
        dst = [ps.pool_alloc(n * 4) for _ in range(2)]
        third = ps.pool_alloc(n * 4)
        pay = _payload(5, 2, n)
        for b, v in zip(src, pay):
            b.copy_from(v)
        for _ in range(2):  # learn the advert, then one fused round
            worker.round_mixed(key, [src[0].ptr], [dst[0].ptr], [n * 4], 0, 1, True)
        dst[0].copy_from(np.zeros(n, dtype=np.float32))
        c0 = ps._core.fused_assign_count()
        ts = [worker.zpushpull_ptr(key, src[i].ptr, dst[i].ptr, n * 4, 0, lens, cmd=1)
              for i in range(2)]
        for t in ts:
            worker.wait(t)
        assert ps._core.fused_assign_count() - c0 == 2
        assert np.array_equal(dst[0].to_numpy_f32(), pay[0])
        assert np.array_equal(dst[1].to_numpy_f32(), pay[1])
        worker.wait(worker.zpull_ptr(key, third.ptr, n * 4, 0, lens, cmd=1))
        assert np.array_equal(third.to_numpy_f32(), pay[1])
    finally:
        _down_joint()


def test_plain_pull_behind_open_batch():
    _boot_joint_inproc(hold=True)
    try:
        server = ps.KVServer(0)
        server.set_gpu_dense_handle(mode="assign")
        worker = ps.KVWorker(0, 0)
        n = _N
        key = np.array([7300], dtype=np.uint64)
        lens = np.array([n], dtype=np.int32)
        src, dst, third = (ps.pool_alloc(n * 4) for _ in range(3))
        old, new = _payload(1, 1, n)[0], _payload(2, 1, n)[0]
        src.copy_from(old)
        for _ in range(2):
            worker.round_mixed(key, [src.ptr], [dst.ptr], [n * 4], 0, 1, True)
        src.copy_from(new)
        third.copy_from(np.zeros(n, dtype=np.float32))
        c0 = ps._core.fused_assign_count()
        t_fused = worker.zpushpull_ptr(key, src.ptr, dst.ptr, n * 4, 0, lens, cmd=1)
        t_pull = worker.zpull_ptr(key, third.ptr, n * 4, 0, lens, cmd=1)
        worker.wait(t_pull)
        assert np.array_equal(third.to_numpy_f32(), new)
        worker.wait(t_fused)
        assert ps._core.fused_assign_count() - c0 == 1
        assert np.array_equal(dst.to_numpy_f32(), new)
    finally:
        _down_joint()


# ----------------------------------------------------------------- bypasses

def test_tail_key_mixed_into_burst():
    """A 4099-float key (12-byte tail) cannot ride the 16 B batched kernel:
    it flushes the open batch and takes its own launch; values stay right."""
    _boot_joint_inproc(hold=True)
    try:
        server = ps.KVServer(0)
        server.set_gpu_dense_handle(mode="assign")
        worker = ps.KVWorker(0, 0)
        keys = np.arange(7400, 7407, dtype=np.uint64)
        sizes = [_N, _N, _N, 4099, _N, _N, _N]
        deltas, _ = _rounds(ps, worker, keys, sizes)
        for kd, ld in deltas[1:]:
            # {3 keys}, the tail key alone, {3 keys}
            assert kd == 7 and 3 <= ld <= 7, deltas
    finally:
        _down_joint()


def _switch_off_fn(ps_mod, rank):
    server = ps_mod.KVServer(0)
    server.set_gpu_dense_handle(mode="assign")
    worker = ps_mod.KVWorker(0, 0)
    keys = np.arange(7500, 7510, dtype=np.uint64)
    deltas, _ = _rounds(ps_mod, worker, keys, [_N] * 10)
    return [list(map(int, d)) for d in deltas], server


def test_coalesce_switch_off_in_child():
    """XPS_COALESCE=0: one launch per key again, values checked in the child."""
    results = launch_local(1, 1, _switch_off_fn, joint=True, devices={0: 0},
                           env_extra={"XPS_POOL_GB": 4, "XPS_COALESCE": 0, _HOLD: 1},
                           timeout=300)
    deltas = results[0]
    assert deltas[0][0] == 0
    for kd, ld in deltas[1:]:
        assert kd == 10 and ld == 10, deltas


# ----------------------------------------------------------- cross-process

def _cross_worker_fn(ps_mod, rank):
    """Two joint processes on one GPU, 8 single-writer keys per rank: 4 on
    the rank's own server (handler launches) and 4 on the other one (the
    worker's one-sided EntryPushPull from step 2 on)."""
    server = ps_mod.KVServer(0)
    server.set_gpu_dense_handle(mode="assign")
    ps_mod.barrier("worker", ps_mod.WORKER_GROUP)
    worker = ps_mod.KVWorker(0, 0)
    keys = np.array([1000 + 10 * rank + i for i in range(4)] +
                    [_HALF + 2000 + 10 * rank + i for i in range(4)], dtype=np.uint64)
    deltas, _ = _rounds(ps_mod, worker, keys, [_N] * 8, salt=100000.0 * (rank + 1))
    ps_mod.barrier("worker", ps_mod.WORKER_GROUP)
    return [list(map(int, d)) for d in deltas], server


def test_coalesced_cross_process():
    results = launch_local(2, 2, _cross_worker_fn, joint=True, devices={0: 0, 1: 0},
                           env_extra={"XPS_POOL_GB": 4, _HOLD: 1,
                                      "XPS_COALESCE_ONE_SIDED": 1}, timeout=300)
    assert len(results) == 2
    for rank, deltas in results.items():
        for kd, ld in deltas[1:]:
            assert kd > 0 and ld < kd, results
