"""MXFP8 on the MI355X: the kernels of csrc/mxfp8.hip against the host
reference and the torch model (mxfp8_model.py), then the reduce-mode dense
handler and PSGradSync on packed payloads end to end. All marked gpu."""
import threading

import numpy as np
import pytest
import torch

import mxfp8_model as model
import ps_lite_amd as ps
from ps_lite_amd import ops
from ps_lite_amd.parallel import launch_local

pytestmark = pytest.mark.gpu

_core = ps._core
_PORT = [31900]
_GUARD = 528  # guard bytes either side of every output (a 16 B multiple)
_FILL = 0xA5


def _data(n, seed):
    """Half Gaussian, half heavy-tailed, with a run of zeros."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    heavy = x * torch.exp(3 * torch.randn(n, generator=g))
    x = torch.where(torch.arange(n) % 2 == 0, x, heavy)
    x[n // 3:n // 3 + 40] = 0.0
    return x


def _packed_model(x):
    return model.pack(*model.quantize(x))


def _guarded_bytes(nbytes):
    """(whole buffer, the nbytes in the middle) of a 0xA5-filled device buffer."""
    whole = torch.full((_GUARD + nbytes + _GUARD,), _FILL, dtype=torch.uint8, device="cuda:0")
    return whole, whole[_GUARD:_GUARD + nbytes]


def _guards_intact(whole, nbytes):
    w = whole.cpu()
    return bool((w[:_GUARD] == _FILL).all()) and bool((w[_GUARD + nbytes:] == _FILL).all())


def _guarded_f32(n, off):
    """n floats starting off elements past a 16 B boundary, fenced by
    sentinels; off = 1 puts the pointer 4 bytes off alignment."""
    whole = torch.full((8 + n + 8,), -7.5, device="cuda:0")
    view = whole[4 + off:4 + off + n]
    assert view.data_ptr() % 16 == 4 * off
    return whole, view


def _f32_guards_intact(whole, n, off):
    w = whole.cpu()
    return bool((w[:4 + off] == -7.5).all()) and bool((w[4 + off + n:] == -7.5).all())


def _f32_src(x, off):
    buf = torch.zeros(4 + off + x.numel(), device="cuda:0")
    view = buf[4 + off:]
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 * off
    return buf, view


# ---------------------------------------------------------------- kernels


@pytest.mark.parametrize("n", [1, 33, 511, 513, 1041, 8 * 512, 70001])
def test_quantize_dequantize_kernels(n):
    x = _data(n, seed=n)
    nbytes = model.packed_nbytes(n)
    want_packed = _packed_model(x)
    host_packed = _core.mxfp8_quantize_host(x.numpy())
    model.assert_packed_equal(host_packed, want_packed, "host reference")
    byte, codes = model.quantize(x)
    want = model.dequantize(byte, codes, n)
    want_third = model.dequantize(byte, codes, n, alpha=1.0 / 3.0)
    packed_dev = want_packed.to("cuda:0")
    for grid_cap in (1, 0):
        for off in (0, 1):
            what = f"n={n} grid_cap={grid_cap} off={off}"
            keep, src = _f32_src(x, off)
            whole, out = _guarded_bytes(nbytes)
            _core.k_mx_quantize(src.data_ptr(), n, out.data_ptr(), grid_cap=grid_cap)
            assert _guards_intact(whole, nbytes), what
            model.assert_packed_equal(out.cpu().numpy(), want_packed, what)
            # zero fill past n: the padding's codes are zeros
            gb, gc = model.unpack(out.cpu().numpy())
            assert not model.dequantize(gb, gc, gb.numel() * 32)[n:].any(), what

            dwhole, dst = _guarded_f32(n, off)
            _core.k_mx_dequantize(packed_dev.data_ptr(), n, dst.data_ptr(), grid_cap=grid_cap)
            assert _f32_guards_intact(dwhole, n, off), what
            assert torch.equal(dst.cpu(), want), what
            _core.k_mx_dequantize(packed_dev.data_ptr(), n, dst.data_ptr(), alpha=1.0 / 3.0,
                                  grid_cap=grid_cap)
            assert _f32_guards_intact(dwhole, n, off), what
            assert torch.equal(dst.cpu(), want_third), what


def test_ops_wrappers():
    n = 1041
    x = _data(n, seed=5)
    packed = ops.mxfp8_quantize(x.to("cuda:0"))
    assert packed.dtype == torch.uint8 and packed.numel() == ops.mxfp8_packed_nbytes(n)
    model.assert_packed_equal(packed.cpu().numpy(), _packed_model(x))
    assert torch.equal(ops.mxfp8_dequantize(packed, n).cpu(), model.roundtrip(x))
    out = torch.empty(n, device="cuda:0")
    assert ops.mxfp8_dequantize(packed, n, alpha=0.5, out=out) is out
    assert torch.equal(out.cpu(), model.roundtrip(x) * 0.5)


def _three_payloads(nsb, seed):
    n = nsb * 512
    xs = [_data(n, seed=seed + i) for i in range(3)]
    packed = [_packed_model(x) for x in xs]
    vals = [model.roundtrip(x) for x in xs]
    return n, packed, vals


@pytest.mark.parametrize("nsb", [1, 3, 137])
@pytest.mark.parametrize("off", [0, 1])
def test_accumulate_and_finish_kernels(nsb, off):
    n, packed, vals = _three_payloads(nsb, seed=100 + nsb)
    nbytes = nsb * 528
    pa, pb, pc = (p.to("cuda:0") for p in packed)
    whole, acc = _guarded_f32(n, off)
    _core.k_mx_accumulate(acc.data_ptr(), pa.data_ptr(), nbytes, True, grid_cap=1)
    assert torch.equal(acc.cpu(), vals[0])
    _core.k_mx_accumulate(acc.data_ptr(), pb.data_ptr(), nbytes, False, grid_cap=1)
    two = vals[0] + vals[1]
    assert torch.equal(acc.cpu(), two)
    assert _f32_guards_intact(whole, n, off)

    owhole, out = _guarded_bytes(nbytes)
    _core.k_mx_finish(acc.data_ptr(), pc.data_ptr(), out.data_ptr(), nbytes, grid_cap=1)
    assert _guards_intact(owhole, nbytes)
    model.assert_packed_equal(out.cpu().numpy(), _packed_model(two + vals[2]), "finish")
    assert torch.equal(acc.cpu(), two), "finish must not write acc"
    assert _f32_guards_intact(whole, n, off)

    owhole, out = _guarded_bytes(nbytes)
    _core.k_mx_finish(0, pc.data_ptr(), out.data_ptr(), nbytes, grid_cap=1)
    assert _guards_intact(owhole, nbytes)
    model.assert_packed_equal(out.cpu().numpy(), _packed_model(vals[2]), "finish, no acc")


@pytest.mark.parametrize("sizes,tile_cap,launches", [
    ([1, 8, 2, 37], 0, 1),
    ([1, 8, 2, 37], 1, 1),
    ([1, 0, 8, 2, 37], 3, 1),  # an empty segment is skipped
    ([1] * 65, 0, 2),
    ([1] * 65, 1, 2),
])
def test_batched_kernels(sizes, tile_cap, launches):
    segs = []
    for i, nsb in enumerate(sizes):
        n, packed, vals = _three_payloads(nsb, seed=1000 + 3 * i)
        dev = [p.to("cuda:0") for p in packed]
        acc_whole, acc = _guarded_f32(n, 0)
        out_whole, out = _guarded_bytes(nsb * 528)
        segs.append(dict(n=n, nbytes=nsb * 528, dev=dev, vals=vals, acc_whole=acc_whole, acc=acc,
                         out_whole=out_whole, out=out))

    def tuples(which):
        return [(s["acc"].data_ptr(), s["dev"][which].data_ptr(), s["out"].data_ptr(), s["nbytes"])
                for s in segs]

    assert _core.k_batched_mx_accumulate(tuples(0), True, tile_cap=tile_cap) == launches
    for s in segs:
        assert torch.equal(s["acc"].cpu(), s["vals"][0])
    assert _core.k_batched_mx_accumulate(tuples(1), False, tile_cap=tile_cap) == launches
    for s in segs:
        assert torch.equal(s["acc"].cpu(), s["vals"][0] + s["vals"][1])
        assert _guards_intact(s["out_whole"], s["nbytes"])
        assert bool((s["out"] == _FILL).all()), "accumulate must not write out"
    assert _core.k_batched_mx_finish(tuples(2), tile_cap=tile_cap) == launches
    for s in segs:
        two = s["vals"][0] + s["vals"][1]
        if s["nbytes"]:
            model.assert_packed_equal(s["out"].cpu().numpy(), _packed_model(two + s["vals"][2]))
        assert torch.equal(s["acc"].cpu(), two)
        assert _guards_intact(s["out_whole"], s["nbytes"])
        assert _f32_guards_intact(s["acc_whole"], s["n"], 0)
    # no accumulator: out = Q(D(in))
    no_acc = [(0, s["dev"][2].data_ptr(), s["out"].data_ptr(), s["nbytes"]) for s in segs]
    assert _core.k_batched_mx_finish(no_acc, tile_cap=tile_cap) == launches
    for s in segs:
        if s["nbytes"]:
            model.assert_packed_equal(s["out"].cpu().numpy(), _packed_model(s["vals"][2]))


def test_bad_packed_arguments_launch_nothing():
    nbytes = 2 * 528
    whole, out = _guarded_bytes(nbytes + 16)
    packed = _packed_model(_data(1024, seed=9)).to("cuda:0")
    spare = torch.cat([packed, packed])  # room for a pointer 8 bytes in
    acc = torch.full((1024,), -7.5, device="cuda:0")
    src = torch.ones(1024, device="cuda:0")
    p, o = packed.data_ptr(), out.data_ptr()
    with pytest.raises(ValueError):
        _core.k_mx_quantize(src.data_ptr(), 1024, o + 8)
    with pytest.raises(ValueError):
        _core.k_mx_dequantize(spare.data_ptr() + 8, 1024, acc.data_ptr())
    for bad_ptr, bad_len in ((spare.data_ptr() + 8, nbytes), (p, nbytes - 1), (p, nbytes + 16)):
        with pytest.raises(ValueError):
            _core.k_mx_accumulate(acc.data_ptr(), bad_ptr, bad_len, True)
        with pytest.raises(ValueError):
            _core.k_mx_finish(acc.data_ptr(), bad_ptr, o, bad_len)
        with pytest.raises(ValueError):
            _core.k_batched_mx_accumulate([(acc.data_ptr(), p, o, 528),
                                           (acc.data_ptr(), bad_ptr, o, bad_len)], True)
        with pytest.raises(ValueError):
            _core.k_batched_mx_finish([(0, p, o, 528), (0, bad_ptr, o, bad_len)])
    with pytest.raises(ValueError):
        _core.k_mx_finish(0, p, o + 8, nbytes)
    ps.device_sync(0)
    assert bool((whole == _FILL).all()) and bool((acc == -7.5).all())


# ------------------------------------------------------------- end to end


def _bytes_of(buf, nbytes):
    """A pool buffer's first nbytes as a uint8 array (bit-preserving)."""
    return buf.to_numpy_f32().view(np.uint8)[:nbytes].copy()


def _rank_step_packed(rank, step, lens_sb):
    """Host-side packed payload of one rank and step: one segment per key."""
    return [_core.mxfp8_quantize_host(_data(nsb * 512, seed=7919 * rank + 31 * step + i).numpy())
            for i, nsb in enumerate(lens_sb)]


def _expected_two_worker(step, lens_sb):
    out = []
    for i, nsb in enumerate(lens_sb):
        vals = [model.roundtrip(_data(nsb * 512, seed=7919 * rank + 31 * step + i))
                for rank in (0, 1)]
        out.append(_packed_model(vals[0] + vals[1]))
    return torch.cat(out)


def test_reduce_mxfp8_one_joint_process():
    """One worker: each round is the finish kernel alone, so the pull
    returns Q(D(p)), which dequantizes to D(Q(D(p)))."""
    _PORT[0] += 7
    ps.setup_env(1, 1, root_port=_PORT[0], XPS_DEV_ID=0, XPS_POOL_GB=4)
    roles = (("scheduler", -1), ("joint", 0))
    ths = [threading.Thread(target=ps.start, kwargs=dict(role=r, device=d)) for r, d in roles]
    [t.start() for t in ths]
    [t.join() for t in ths]
    try:
        server = ps.KVServer(0)
        server.set_gpu_dense_handle(mode="reduce", dtype="mxfp8")
        worker = ps.KVWorker(0, 0)
        nsb, n = 3, 3 * 512
        nbytes = nsb * 528
        src, dst = ps.pool_alloc(nbytes), ps.pool_alloc(nbytes)
        keys = np.array([5], dtype=np.uint64)
        lens = np.array([nbytes // 4], dtype=np.int32)
        before = _core.mxfp8_launches()
        for step in range(2):
            x = _data(n, seed=40 + step)
            p = _packed_model(x)
            src.copy_from(p.numpy())
            ts1 = worker.zpush_ptr(keys, src.ptr, nbytes, 0, lens)
            ts2 = worker.zpull_ptr(keys, dst.ptr, nbytes, 0, lens)
            worker.wait(ts1)
            worker.wait(ts2)
            got = _bytes_of(dst, nbytes)
            model.assert_packed_equal(got, _packed_model(model.roundtrip(x)), f"step {step}")
            gb, gc = model.unpack(got)
            assert torch.equal(model.dequantize(gb, gc, n), model.roundtrip(model.roundtrip(x)))
        assert _core.mxfp8_launches() - before == 2
    finally:
        ths = [threading.Thread(target=ps.finalize, kwargs=dict(role=r)) for r, _ in roles]
        [t.start() for t in ths]
        [t.join() for t in ths]
        ps.clear_registry()


def _mx_reduce_worker_fn(ps_mod, rank, lens_sb):
    server = ps_mod.KVServer(0)
    server.set_gpu_dense_handle(mode="reduce", dtype="mxfp8")
    ps_mod.barrier("worker", ps_mod.WORKER_GROUP)
    worker = ps_mod.KVWorker(0, 0)
    total = sum(lens_sb) * 528
    src = ps_mod.pool_alloc(total)
    dst = ps_mod.pool_alloc(total)
    keys = np.arange(61, 61 + len(lens_sb), dtype=np.uint64)
    lens = np.array([nsb * 132 for nsb in lens_sb], dtype=np.int32)
    outs = []
    for step in range(4):  # several rounds: reset, deferred pushes
        src.copy_from(np.concatenate(_rank_step_packed(rank, step, lens_sb)))
        ts1 = worker.zpush_ptr(keys, src.ptr, total, 0, lens)
        ts2 = worker.zpull_ptr(keys, dst.ptr, total, 0, lens)  # overlapped, no barrier
        worker.wait(ts1)
        worker.wait(ts2)
        outs.append(_bytes_of(dst, total))
    # this process's server side: every launch since the process began (a
    # pull completes only after both pushes of its round were handled)
    return (outs, int(ps_mod._core.mxfp8_launches())), server


def _check_two_worker_rounds(results, lens_sb):
    for step in range(4):
        want = _expected_two_worker(step, lens_sb)
        for rank in (0, 1):
            outs, _ = results[rank]
            at = 0
            for nsb in lens_sb:  # per key, so a failure names its segment
                seg = slice(at, at + nsb * 528)
                model.assert_packed_equal(outs[step][seg], want[seg], f"step {step} rank {rank}")
                at += nsb * 528


def test_reduce_mxfp8_two_joint_on_one_gpu():
    """Two workers, one key, 4 overlapped rounds: both pull Q(D(pa) + D(pb)).
    Two addends commute, so the arrival order cannot change a bit."""
    lens_sb = [3]
    results = launch_local(2, 2, _mx_reduce_worker_fn, joint=True, devices={0: 0, 1: 0},
                           env_extra={"XPS_POOL_GB": 4}, timeout=300, worker_args=(lens_sb,))
    _check_two_worker_rounds(results, lens_sb)
    assert results[0][1] + results[1][1] == 8, (results[0][1], results[1][1])


def test_reduce_mxfp8_multikey_two_joint_on_one_gpu():
    """4 keys in one message: one accumulate or finish launch per push."""
    lens_sb = [1, 8, 2, 37]
    results = launch_local(2, 2, _mx_reduce_worker_fn, joint=True, devices={0: 0, 1: 0},
                           env_extra={"XPS_POOL_GB": 4}, timeout=300, worker_args=(lens_sb,))
    _check_two_worker_rounds(results, lens_sb)
    # the four keys share one server and one message: 4 rounds x 2 pushes
    # make 8 launches over both processes, one per push, not 32
    assert results[0][1] + results[1][1] == 8, (results[0][1], results[1][1])


def test_gradsync_mxfp8():
    from ps_lite_amd.parallel.dp import PSGradSync

    _PORT[0] += 7
    ps.setup_env(1, 1, root_port=_PORT[0], XPS_DEV_ID=0, XPS_POOL_GB=4)
    roles = (("scheduler", -1), ("joint", 0))
    ths = [threading.Thread(target=ps.start, kwargs=dict(role=r, device=d)) for r, d in roles]
    [t.start() for t in ths]
    [t.join() for t in ths]
    try:
        server = ps.KVServer(0)
        server.set_gpu_dense_handle(mode="reduce", dtype="mxfp8")
        worker = ps.KVWorker(0, 0)
        params = [torch.nn.Parameter(torch.zeros(n, device="cuda:0")) for n in (1000, 37, 513)]
        sync = PSGradSync(ps, worker, params, num_workers=1, device=0, compress="mxfp8")
        for step in range(2):
            grads = [_data(p.numel(), seed=300 + 10 * step + i) for i, p in enumerate(params)]
            for p, g in zip(params, grads):
                p.grad = g.to("cuda:0")
            sync.allreduce()
            torch.cuda.synchronize()
            for p, g in zip(params, grads):
                # worker Q, server Q(D(.)), worker D with alpha = 1/1
                once = model.roundtrip(g)
                assert torch.equal(p.grad.cpu(), model.roundtrip(once))
                assert torch.equal(model.roundtrip(once), once)
                # within block amax / 16 twice over of the uncompressed grad;
                # and with one worker within amax / 16 once, since the
                # server's rounding of D(Q(g)) is exact (value idempotence,
                # asserted just above)
                pad = -g.numel() % 32
                amax = torch.cat([g, torch.zeros(pad)]).view(-1, 32).abs().amax(dim=1)
                amax = amax.repeat_interleave(32)[:g.numel()]
                err = (p.grad.cpu() - g).abs()
                assert bool((err <= amax / 8).all())
                assert bool((err <= amax / 16).all())
    finally:
        ths = [threading.Thread(target=ps.finalize, kwargs=dict(role=r)) for r, _ in roles]
        [t.start() for t in ths]
        [t.join() for t in ths]
        ps.clear_registry()


def test_gradsync_compress_none_is_the_fp32_path():
    """compress=None is PSGradSync as it was (the flow of
    test_dp_gradsync_gpu): one worker gets its own grads back."""
    from ps_lite_amd.parallel.dp import PSGradSync

    _PORT[0] += 7
    ps.setup_env(1, 1, root_port=_PORT[0], XPS_DEV_ID=0, XPS_POOL_GB=4)
    roles = (("scheduler", -1), ("joint", 0))
    ths = [threading.Thread(target=ps.start, kwargs=dict(role=r, device=d)) for r, d in roles]
    [t.start() for t in ths]
    [t.join() for t in ths]
    try:
        server = ps.KVServer(0)
        server.set_gpu_dense_handle(mode="reduce")
        worker = ps.KVWorker(0, 0)
        torch.manual_seed(0)
        net = torch.nn.Linear(64, 32).cuda()
        sync = PSGradSync(ps, worker, net.parameters(), num_workers=1, device=0, compress=None)
        before_launches = _core.mxfp8_launches()
        for step in range(3):
            x = torch.randn(16, 64, device="cuda:0")
            net.zero_grad()
            net(x).sum().backward()
            before = [p.grad.clone() for p in net.parameters()]
            sync.allreduce()
            torch.cuda.synchronize()
            for b, p in zip(before, net.parameters()):
                assert torch.allclose(b, p.grad, atol=1e-6)
        assert _core.mxfp8_launches() == before_launches
    finally:
        ths = [threading.Thread(target=ps.finalize, kwargs=dict(role=r)) for r, _ in roles]
        [t.start() for t in ths]
        [t.join() for t in ths]
        ps.clear_registry()
