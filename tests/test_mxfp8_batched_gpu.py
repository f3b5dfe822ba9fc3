"""The batched worker-side MXFP8 pair on the MI355X (BatchedMxQuantize /
BatchedMxDequantize in csrc/mxfp8.hip): against the torch model
(mxfp8_model.py) and the single kernels, then through the ops wrappers and
PSGradSync. Every comparison is exact. All marked gpu."""
import functools
import threading

import pytest
import torch

import mxfp8_model as model
import ps_lite_amd as ps
from ps_lite_amd import ops

pytestmark = pytest.mark.gpu

_core = ps._core
_PORT = [32300]
_GUARD = 528  # guard bytes either side of every packed output (a 16 B multiple)
_FILL = 0xA5
_SENTINEL = -7.5


def _data(n, seed):
    """Half Gaussian, half heavy-tailed, with a run of zeros."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    heavy = x * torch.exp(3 * torch.randn(n, generator=g))
    x = torch.where(torch.arange(n) % 2 == 0, x, heavy)
    x[n // 3:n // 3 + 40] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def _ref(n, seed):
    """(x, packed model, D(Q(x)), D(Q(x)) / 3) on the CPU; computed once per
    (n, seed), shared by every test and never written to."""
    x = _data(n, seed)
    byte, codes = model.quantize(x)
    return (x, model.pack(byte, codes), model.dequantize(byte, codes, n),
            model.dequantize(byte, codes, n, alpha=1.0 / 3.0))


def _guarded_bytes(nbytes):
    whole = torch.full((_GUARD + nbytes + _GUARD,), _FILL, dtype=torch.uint8, device="cuda:0")
    return whole, whole[_GUARD:_GUARD + nbytes]


def _guards_intact(whole, nbytes):
    w = whole.cpu()
    return bool((w[:_GUARD] == _FILL).all()) and bool((w[_GUARD + nbytes:] == _FILL).all())


def _guarded_f32(n, off):
    """n floats starting off elements past a 16 B boundary, fenced by
    sentinels; off = 1 puts the pointer 4 bytes off alignment."""
    whole = torch.full((8 + n + 8,), _SENTINEL, device="cuda:0")
    view = whole[4 + off:4 + off + n]
    assert view.data_ptr() % 16 == 4 * off
    return whole, view


def _f32_guards_intact(whole, n, off):
    w = whole.cpu()
    return bool((w[:4 + off] == _SENTINEL).all()) and bool((w[4 + off + n:] == _SENTINEL).all())


def _f32_src(x, off):
    buf = torch.zeros(4 + off + x.numel(), device="cuda:0")
    view = buf[4 + off:]
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 * off
    return buf, view


def _same_bits(a, b):
    return torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


# ---------------------------------------------------------------- kernels

_MIXED = [1, 33, 511, 513, 1041, 4096, 70001]


@pytest.mark.parametrize("tile_cap", [0, 1, 3])
@pytest.mark.parametrize("misaligned", [False, True])
def test_mixed_list(tile_cap, misaligned):
    """Seven segments, 1 to 70001 elements, in one launch. misaligned puts
    segment 2 four bytes off a 16 B boundary, which makes the whole launch
    element-wise."""
    offs = [1 if misaligned and i == 2 else 0 for i in range(len(_MIXED))]
    segs = []
    for n, off in zip(_MIXED, offs):
        x, want_packed, want, want_third = _ref(n, n)
        nbytes = model.packed_nbytes(n)
        keep, src = _f32_src(x, off)
        whole, out = _guarded_bytes(nbytes)
        dwhole, dst = _guarded_f32(n, off)
        segs.append(dict(n=n, off=off, nbytes=nbytes, keep=keep, src=src, whole=whole, out=out,
                         dwhole=dwhole, dst=dst, packed_dev=want_packed.to("cuda:0")))

    got = _core.k_batched_mx_quantize([(s["src"].data_ptr(), s["out"].data_ptr(), s["n"])
                                       for s in segs], tile_cap=tile_cap)
    assert got == 1
    for s in segs:
        n, what = s["n"], f"n={s['n']} tile_cap={tile_cap} off={s['off']}"
        want_packed = _ref(n, n)[1]
        assert _guards_intact(s["whole"], s["nbytes"]), what
        model.assert_packed_equal(s["out"].cpu().numpy(), want_packed, what)
        single = torch.empty(s["nbytes"], dtype=torch.uint8, device="cuda:0")
        _core.k_mx_quantize(s["src"].data_ptr(), n, single.data_ptr())
        assert torch.equal(s["out"], single), what
        # zero fill past n: the padding's codes are zeros
        gb, gc = model.unpack(s["out"].cpu().numpy())
        assert not model.dequantize(gb, gc, gb.numel() * 32)[n:].any(), what

    dq = [(s["dst"].data_ptr(), s["packed_dev"].data_ptr(), s["n"]) for s in segs]
    for alpha, which in ((1.0, 2), (1.0 / 3.0, 3)):
        assert _core.k_batched_mx_dequantize(dq, alpha=alpha, tile_cap=tile_cap) == 1
        for s in segs:
            n, what = s["n"], f"n={s['n']} tile_cap={tile_cap} off={s['off']} alpha={alpha}"
            assert _f32_guards_intact(s["dwhole"], n, s["off"]), what
            assert torch.equal(s["dst"].cpu(), _ref(n, n)[which]), what
            single = torch.empty(n, device="cuda:0")
            _core.k_mx_dequantize(s["packed_dev"].data_ptr(), n, single.data_ptr(), alpha=alpha)
            assert _same_bits(s["dst"], single), what


@pytest.mark.parametrize("lens", [(37, 1000, 513, 25), (1000, 516, 40)])
def test_neighbouring_buckets(lens):
    """Consecutive slices of one fp32 tensor, as gradient buckets of one
    parameter are. (37, 1000, 513, 25) start at 0, 37, 1037, 1550: three
    starts off alignment and no end on a quad boundary. (1000, 516, 40)
    start at 0, 1000, 1516: 16 B-aligned starts and quad-aligned ends inside
    a superblock, so the float4 kernels run with in-superblock tails."""
    total = sum(lens)
    starts = [sum(lens[:i]) for i in range(len(lens))]
    refs = [_ref(n, 50 + i) for i, n in enumerate(lens)]
    aligned = all(4 * s % 16 == 0 for s in starts)
    assert aligned == (lens == (1000, 516, 40))

    # dequantize into the slices of a sentinel-filled tensor
    whole = torch.full((8 + total + 8,), _SENTINEL, device="cuda:0")
    assert whole[4:].data_ptr() % 16 == 0
    views = [whole[4 + s:4 + s + n] for s, n in zip(starts, lens)]
    packed = [r[1].to("cuda:0") for r in refs]
    for alpha, which in ((1.0, 2), (1.0 / 3.0, 3)):
        segs = [(v.data_ptr(), p.data_ptr(), n) for v, p, n in zip(views, packed, lens)]
        assert _core.k_batched_mx_dequantize(segs, alpha=alpha) == 1
        for i, v in enumerate(views):
            assert torch.equal(v.cpu(), refs[i][which]), (lens, i, alpha)
        assert _f32_guards_intact(whole, total, 0)

    # the same layout as the quantize source
    src_whole = torch.zeros(4 + total, device="cuda:0")
    src_whole[4:].copy_(torch.cat([r[0] for r in refs]))
    outs = [_guarded_bytes(model.packed_nbytes(n)) for n in lens]
    segs = [(src_whole[4 + s:].data_ptr(), o[1].data_ptr(), n)
            for s, o, n in zip(starts, outs, lens)]
    assert _core.k_batched_mx_quantize(segs) == 1
    for i, (owhole, out) in enumerate(outs):
        assert _guards_intact(owhole, out.numel()), (lens, i)
        model.assert_packed_equal(out.cpu().numpy(), refs[i][1], f"{lens} segment {i}")
        single = torch.empty_like(out)
        _core.k_mx_quantize(segs[i][0], lens[i], single.data_ptr())
        assert torch.equal(out, single), (lens, i)


@pytest.mark.parametrize("tile_cap", [0, 1])
@pytest.mark.parametrize("with_empty", [False, True])
def test_more_than_one_launch_and_empty_segments(tile_cap, with_empty):
    """65 segments of 40 elements need two launches; an empty segment in the
    middle is skipped and counts towards neither launch."""
    n, count = 40, 65
    x = _ref(n * count, 77)[0]
    chunks = list(x.split(n))
    want_packed = [model.pack(*model.quantize(c)) for c in chunks]
    want = [model.roundtrip(c) for c in chunks]
    src = x.to("cuda:0")
    # packed outputs 528 bytes each, 528 bytes of fill between them
    out_all = torch.full((count * 1056 + 528,), _FILL, dtype=torch.uint8, device="cuda:0")
    outs = [out_all[528 + i * 1056:528 + i * 1056 + 528] for i in range(count)]
    assert all(o.data_ptr() % 16 == 0 for o in outs)
    qsegs = [(src[i * n:].data_ptr(), outs[i].data_ptr(), n) for i in range(count)]
    packed_dev = [p.to("cuda:0") for p in want_packed]
    dst_all = torch.full((count * (n + 3) + 3,), _SENTINEL, device="cuda:0")
    dsts = [dst_all[3 + i * (n + 3):3 + i * (n + 3) + n] for i in range(count)]
    dsegs = [(dsts[i].data_ptr(), packed_dev[i].data_ptr(), n) for i in range(count)]
    if with_empty:
        e_f32 = torch.full((16,), _SENTINEL, device="cuda:0")
        e_packed = torch.full((528,), _FILL, dtype=torch.uint8, device="cuda:0")
        qsegs.insert(30, (e_f32.data_ptr(), e_packed.data_ptr(), 0))
        dsegs.insert(30, (e_f32.data_ptr(), e_packed.data_ptr(), 0))

    assert _core.k_batched_mx_quantize(qsegs, tile_cap=tile_cap) == 2
    got = out_all.cpu()
    fill = torch.ones(out_all.numel(), dtype=torch.bool)
    for i in range(count):
        at = 528 + i * 1056
        model.assert_packed_equal(got[at:at + 528].numpy(), want_packed[i], f"segment {i}")
        fill[at:at + 528] = False
    assert bool((got[fill] == _FILL).all())

    assert _core.k_batched_mx_dequantize(dsegs, tile_cap=tile_cap) == 2
    got = dst_all.cpu()
    fill = torch.ones(dst_all.numel(), dtype=torch.bool)
    for i in range(count):
        at = 3 + i * (n + 3)
        assert torch.equal(got[at:at + n], want[i]), f"segment {i}"
        fill[at:at + n] = False
    assert bool((got[fill] == _SENTINEL).all())
    if with_empty:
        assert bool((e_f32 == _SENTINEL).all()) and bool((e_packed == _FILL).all())


def test_bad_arguments_launch_nothing():
    n = 1024
    nbytes = model.packed_nbytes(n)
    whole, out = _guarded_bytes(2 * nbytes + 16)
    packed = _ref(n, 9)[1].to("cuda:0")
    spare = torch.cat([packed, packed])  # room for a pointer 8 bytes in
    dst = torch.full((2 * n,), _SENTINEL, device="cuda:0")
    src = torch.ones(n, device="cuda:0")
    o, p, d, s = out.data_ptr(), packed.data_ptr(), dst.data_ptr(), src.data_ptr()
    with pytest.raises(ValueError):
        _core.k_batched_mx_quantize([(s, o, n), (s, o + nbytes + 8, n)])
    with pytest.raises(ValueError):
        _core.k_batched_mx_quantize([(s, o, n), (0, o + nbytes, n)])
    with pytest.raises(ValueError):
        _core.k_batched_mx_dequantize([(d, p, n), (d + 4 * n, spare.data_ptr() + 8, n)])
    with pytest.raises(ValueError):
        _core.k_batched_mx_dequantize([(d, p, n), (0, p, n)])
    ps.device_sync(0)
    assert bool((whole == _FILL).all()) and bool((dst == _SENTINEL).all())


def test_ops_many_wrappers():
    lens = (37, 1000, 513)
    x = torch.cat([_ref(n, 20 + i)[0] for i, n in enumerate(lens)]).to("cuda:0")
    slices = list(x.split(lens))
    assert [s.data_ptr() % 16 for s in slices] == [0, 4, 4]  # two off alignment
    packed = ops.mxfp8_quantize_many(slices)
    assert len(packed) == 3
    for sl, p in zip(slices, packed):
        assert p.dtype == torch.uint8 and p.numel() == ops.mxfp8_packed_nbytes(sl.numel())
        assert torch.equal(p, ops.mxfp8_quantize(sl))
    back = ops.mxfp8_dequantize_many(packed, lens)
    for sl, p, b in zip(slices, packed, back):
        assert b.dtype == torch.float32 and b.numel() == sl.numel()
        assert _same_bits(b, ops.mxfp8_dequantize(p, sl.numel()))
        assert torch.equal(b.cpu(), model.roundtrip(sl.cpu()))

    # outs= is written and handed back
    outs = [torch.full((ops.mxfp8_packed_nbytes(n),), _FILL, dtype=torch.uint8, device="cuda:0")
            for n in lens]
    got = ops.mxfp8_quantize_many(slices, outs=outs)
    assert all(g is o for g, o in zip(got, outs))
    assert all(torch.equal(o, p) for o, p in zip(outs, packed))
    y = torch.full((sum(lens),), _SENTINEL, device="cuda:0")
    views = list(y.split(lens))
    got = ops.mxfp8_dequantize_many(packed, lens, alpha=0.5, outs=views)
    assert all(g is v for g, v in zip(got, views))
    for v, p, n in zip(views, packed, lens):
        assert _same_bits(v, ops.mxfp8_dequantize(p, n, alpha=0.5))


# ------------------------------------------------------------- end to end


def _roundtrip_buckets(g, elems):
    """D(Q(.)) bucket by bucket: every bucket is a packed payload of its
    own, so its 32-element blocks count from the bucket's first element."""
    return torch.cat([model.roundtrip(c) for c in g.split(elems)])


@pytest.mark.parametrize("sizes,buckets", [((1000, 37, 513), 63), ((1000, 37, 513, 100), 67)])
def test_gradsync_mx_batched(sizes, buckets):
    """25-element buckets (partition_bytes=100), most of them off alignment;
    63 of them fit one launch, 67 need two. The batched sync and the
    per-bucket sync, on disjoint keys, leave the same bits in .grad."""
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
        params = [torch.nn.Parameter(torch.zeros(n, device="cuda:0")) for n in sizes]
        many = PSGradSync(ps, worker, params, num_workers=1, device=0, compress="mxfp8",
                          partition_bytes=100)
        single = PSGradSync(ps, worker, params, num_workers=1, device=0, compress="mxfp8",
                            partition_bytes=100, key_base=2 << 20, mx_batched=False)
        assert many.mx_batched and len(many.buckets) == len(single.buckets) == buckets
        for step in range(2):
            grads = [_data(p.numel(), seed=300 + 10 * step + i) for i, p in enumerate(params)]
            results = []
            for sync, per_step in ((many, 2 * -(-buckets // 64)), (single, 2 * buckets)):
                for p, g in zip(params, grads):
                    p.grad = g.to("cuda:0")
                before = sync.mx_launches
                sync.allreduce()
                torch.cuda.synchronize()
                assert sync.mx_launches - before == per_step
                results.append([p.grad.cpu() for p in params])
            for g, got_many, got_single in zip(grads, *results):
                # worker Q, server Q(D(.)), worker D with alpha = 1/1
                want = _roundtrip_buckets(_roundtrip_buckets(g, 25), 25)
                assert torch.equal(got_many, want)
                assert _same_bits(got_many, got_single)
    finally:
        ths = [threading.Thread(target=ps.finalize, kwargs=dict(role=r)) for r, _ in roles]
        [t.start() for t in ths]
        [t.join() for t in ths]
        ps.clear_registry()
