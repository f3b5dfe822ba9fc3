"""MXFP8 kernels on the MI355X at the format's edges (csrc/mxfp8.hip): every
e4m3 code boundary and tie, the scale bump, the block amax in either lane's
half and in a partial last block, the ends of the contract, all 256 codes
through every decoder, and the non-finite rule. The expectation is the
format stated by hand in mxfp8_model.py (a table of the e4m3 values,
float64, no fp8 cast), which test_mxfp8_format.py holds the torch model and
the host reference to as well. Every comparison is of bytes or of fp32
bits. All marked gpu."""
import functools

import numpy as np
import pytest
import torch

import mxfp8_model as model
import ps_lite_amd as ps
from ps_lite_amd.parallel import launch_local
from test_mxfp8_format import _edge_blocks
from test_mxfp8_gpu import (_data, _f32_guards_intact, _f32_src, _guarded_bytes, _guarded_f32,
                            _guards_intact)

pytestmark = pytest.mark.gpu

_core = ps._core

_OFF_CAP = [(0, 0), (0, 1), (1, 0), (1, 1)]  # fp32 pointer 16 B-aligned or 4 B past; grid/tile cap


@functools.lru_cache(maxsize=None)
def _cases():
    """[(name, x, Q(x), x as an accumulator, Q(acc + 0), Q(D(Q(x))))], all
    expectations hand-stated, computed once and never written to."""
    out = []
    for name, x, want in model.encode_cases(_edge_blocks()):
        assert model.in_contract(x), name
        acc = model.pad_super(x)
        # through the accumulator the kernel adds D(zero codes) = +0.0, and
        # -0.0 + 0.0 is +0.0: the code of an exact -0.0 loses its sign bit
        # (a negative value that rounds to zero keeps it)
        byte, codes = model.unpack(want)
        codes = codes.view(torch.uint8).reshape(-1).clone()
        codes[(acc == 0) & torch.signbit(acc)] = 0
        via_acc = model.pack(byte, codes.view(-1, 32))
        back = model.hand_decode(byte, model.unpack(want)[1].view(torch.uint8)).reshape(-1)
        out.append((name, x, want, acc, via_acc, model.hand_packed(back)))
    return out


def _dev_bytes(t):
    return t.contiguous().to("cuda:0")


def _zeros_packed(nbytes):
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")


def _diff(got, want):
    """Where two packed streams differ, for the assertion message."""
    at = (got != want).nonzero().reshape(-1)[:6].tolist()
    return [(i // 528, i % 528, int(got[i]), int(want[i])) for i in at]


def _assert_bytes(got_dev, want, what):
    got = got_dev.cpu()
    assert torch.equal(got, want), (what, "(superblock, byte, got, want)", _diff(got, want))


# ------------------------------------------------------------------ encode


@pytest.mark.parametrize("off,cap", _OFF_CAP)
def test_encode_single_kernels(off, cap):
    """k_mx_quantize, and k_mx_finish with the input as the accumulator
    (packed input all zero) and as the packed input (no accumulator), on
    every edge input: scale bytes and code bytes exactly, padding past n as
    zero codes under byte 0."""
    for name, x, want, acc, via_acc, again in _cases():
        what = f"{name} off={off} cap={cap}"
        n, nbytes = x.numel(), want.numel()
        keep, src = _f32_src(x, off)
        whole, out = _guarded_bytes(nbytes)
        _core.k_mx_quantize(src.data_ptr(), n, out.data_ptr(), grid_cap=cap)
        assert _guards_intact(whole, nbytes), what
        _assert_bytes(out, want, "quantize " + what)

        keep, a = _f32_src(acc, off)
        whole, out = _guarded_bytes(nbytes)
        _core.k_mx_finish(a.data_ptr(), _zeros_packed(nbytes).data_ptr(), out.data_ptr(), nbytes,
                          grid_cap=cap)
        assert _guards_intact(whole, nbytes), what
        _assert_bytes(out, via_acc, "finish, input in acc " + what)

        whole, out = _guarded_bytes(nbytes)
        _core.k_mx_finish(0, _dev_bytes(want).data_ptr(), out.data_ptr(), nbytes, grid_cap=cap)
        assert _guards_intact(whole, nbytes), what
        _assert_bytes(out, again, "finish, no acc " + what)


@pytest.mark.parametrize("off,cap", _OFF_CAP)
def test_encode_batched_kernels(off, cap):
    """The same through k_batched_mx_quantize and k_batched_mx_finish, every
    edge input a segment of one launch."""
    cases = _cases()
    assert len(cases) <= 64
    segs = []
    for name, x, want, acc, via_acc, again in cases:
        nbytes = want.numel()
        segs.append(dict(src=_f32_src(x, off), acc=_f32_src(acc, off), zero=_zeros_packed(nbytes),
                         packed=_dev_bytes(want), out=[_guarded_bytes(nbytes) for _ in range(3)]))
    assert _core.k_batched_mx_quantize(
        [(s["src"][1].data_ptr(), s["out"][0][1].data_ptr(), c[1].numel())
         for s, c in zip(segs, cases)], tile_cap=cap) == 1
    assert _core.k_batched_mx_finish(
        [(s["acc"][1].data_ptr(), s["zero"].data_ptr(), s["out"][1][1].data_ptr(), c[2].numel())
         for s, c in zip(segs, cases)], tile_cap=cap) == 1
    assert _core.k_batched_mx_finish(
        [(0, s["packed"].data_ptr(), s["out"][2][1].data_ptr(), c[2].numel())
         for s, c in zip(segs, cases)], tile_cap=cap) == 1
    for s, (name, x, want, acc, via_acc, again) in zip(segs, cases):
        what = f"{name} off={off} cap={cap}"
        for (whole, out), expect, kern in zip(s["out"], (want, via_acc, again),
                                              ("quantize", "finish, input in acc",
                                               "finish, no acc")):
            assert _guards_intact(whole, want.numel()), (kern, what)
            _assert_bytes(out, expect, f"batched {kern} {what}")


# ------------------------------------------------------------------ decode

_THIRD = 1.0 / 3.0


@functools.lru_cache(maxsize=None)
def _table(byte):
    """(packed, D, D * fp32(1/3), acc, acc + D) of code_table(byte), by the
    torch model (which test_mxfp8_format.py holds to the hand table)."""
    packed = model.code_table(byte)
    sb, codes = model.unpack(packed)
    n = sb.numel() * 32
    d = model.dequantize(sb, codes, n)
    third = model.dequantize(sb, codes, n, alpha=_THIRD)
    # a known accumulator: -0.0, the value that cancels D exactly, D, D/2,
    # +0.0 and 3 D in turn; 1.0 where D is NaN
    i = torch.arange(n) % 6
    mult = torch.tensor([0.0, -1.0, 1.0, 0.5, 0.0, 3.0])[i]
    acc = torch.where(torch.isnan(d), torch.ones(n), d.abs() * mult * torch.where(
        torch.signbit(d), -1.0, 1.0))
    acc[i == 0] = -0.0
    acc[i == 4] = 0.0
    total = acc + d
    assert bool((total[(i == 1) & ~torch.isnan(d)] == 0).all())
    return packed, d, third, acc, total


@pytest.mark.parametrize("off,cap", _OFF_CAP)
def test_decode_kernels(off, cap):
    """All 256 codes under scale bytes 19, 127 and 220, the zero codes under
    byte 0: k_mx_dequantize and k_batched_mx_dequantize with alpha 1 and
    1/3, k_mx_accumulate and k_batched_mx_accumulate assigning and adding,
    bit for bit against the model, 0x7F and 0xFF as NaN."""
    n = 1024
    tables = [_table(b) for b in model.TABLE_BYTES]
    dev = [_dev_bytes(t[0]) for t in tables]
    for byte, (packed, d, third, acc, total), p in zip(model.TABLE_BYTES, tables, dev):
        what = f"byte={byte} off={off} cap={cap}"
        for alpha, want in ((1.0, d), (_THIRD, third)):
            whole, dst = _guarded_f32(n, off)
            _core.k_mx_dequantize(p.data_ptr(), n, dst.data_ptr(), alpha=alpha, grid_cap=cap)
            assert _f32_guards_intact(whole, n, off), what
            assert model.same_bits_or_nan(dst, want), ("dequantize", alpha, what)
        whole, a = _guarded_f32(n, off)
        _core.k_mx_accumulate(a.data_ptr(), p.data_ptr(), packed.numel(), True, grid_cap=cap)
        assert model.same_bits_or_nan(a, d), ("accumulate, assign", what)
        a.copy_(acc)
        assert torch.equal(a.cpu().view(torch.int32), acc.view(torch.int32))
        _core.k_mx_accumulate(a.data_ptr(), p.data_ptr(), packed.numel(), False, grid_cap=cap)
        assert _f32_guards_intact(whole, n, off), what
        assert model.same_bits_or_nan(a, total), ("accumulate, add", what)

    # batched: the four tables as the segments of one launch
    for alpha, which in ((1.0, 1), (_THIRD, 2)):
        outs = [_guarded_f32(n, off) for _ in tables]
        assert _core.k_batched_mx_dequantize(
            [(o[1].data_ptr(), p.data_ptr(), n) for o, p in zip(outs, dev)], alpha=alpha,
            tile_cap=cap) == 1
        for byte, t, (whole, dst) in zip(model.TABLE_BYTES, tables, outs):
            assert _f32_guards_intact(whole, n, off), (byte, off, cap)
            assert model.same_bits_or_nan(dst, t[which]), ("batched dequantize", alpha, byte, off)
    outs = [_guarded_f32(n, off) for _ in tables]
    segs = [(o[1].data_ptr(), p.data_ptr(), 0, p.numel()) for o, p in zip(outs, dev)]
    assert _core.k_batched_mx_accumulate(segs, True, tile_cap=cap) == 1
    for byte, t, (whole, a) in zip(model.TABLE_BYTES, tables, outs):
        assert model.same_bits_or_nan(a, t[1]), ("batched accumulate, assign", byte, off, cap)
        a.copy_(t[3])
    assert _core.k_batched_mx_accumulate(segs, False, tile_cap=cap) == 1
    for byte, t, (whole, a) in zip(model.TABLE_BYTES, tables, outs):
        assert _f32_guards_intact(whole, n, off), (byte, off, cap)
        assert model.same_bits_or_nan(a, t[4]), ("batched accumulate, add", byte, off, cap)


# -------------------------------------------------------------- non-finite


@functools.lru_cache(maxsize=None)
def _nonfinite():
    """The inputs and hand-stated outputs of the non-finite rule's tests."""
    x, bad, blocks = model.nonfinite_stream()
    finite = model.hand_packed(x)
    want = model.poisoned_packed(finite, blocks)
    # a finish whose packed input carries the rule's blocks (2 and 20) and
    # whose sum overflows fp32 in one element of block 4: 2^127 + 2^127
    acc = model.pad_super(x)
    acc[4 * 32 + 9] = 2.0 ** 127
    byte = torch.zeros(48, dtype=torch.uint8)
    codes = torch.zeros(48, 32, dtype=torch.uint8)
    byte[4], codes[4] = 246, 0x78  # 256 * 2^119 = 2^127 in all 32 places, finite
    packed_in = model.poisoned_packed(model.pack(byte, codes), [2, 20])
    d_in = model.hand_decode(*[t.view(torch.uint8) for t in model.unpack(packed_in)]).reshape(-1)
    total = acc + d_in
    assert bool(torch.isfinite(acc).all()) and bool(torch.isfinite(d_in[4 * 32:5 * 32]).all())
    assert torch.isinf(total[4 * 32 + 9]) and int(torch.isinf(total).sum()) == 1
    ok = torch.where(torch.isfinite(total), total, torch.zeros(()))
    ok[4 * 32:5 * 32] = 0  # 2^127 is past the contract's end; the block is poisoned anyway
    sum_want = model.poisoned_packed(model.hand_packed(ok), [2, 4, 20])
    # Q(D(in)) of the poisoned stream: its finite blocks requantized
    fb, fc = model.unpack(finite)
    again = model.poisoned_packed(
        model.hand_packed(model.hand_decode(fb, fc.view(torch.uint8)).reshape(-1)), blocks)
    return dict(x=x, bad=bad, blocks=blocks, finite=finite, want=want, acc=acc,
                packed_in=packed_in, sum_want=sum_want, again=again)


def test_non_finite_inputs_hold_what_they_claim():
    r = _nonfinite()
    bad = model.pad_super(r["bad"]).view(-1, 32)
    assert (~torch.isfinite(bad).all(dim=1)).nonzero().reshape(-1).tolist() == r["blocks"]
    spots = {(b, e) for b, e in (~torch.isfinite(bad)).nonzero().tolist()}
    assert {(1, 0), (3, 15), (5, 16), (7, 31), (13, 15), (13, 16), (32, 16)} <= spots
    assert torch.isposinf(bad[9, 7]) and torch.isneginf(bad[11, 20]) and torch.isinf(bad[13, 16])
    assert r["bad"].numel() % 512 == 17
    # each poisoned block has finite blocks either side in its superblock
    assert all(b % 16 == 0 or b - 1 not in r["blocks"] for b in r["blocks"])
    assert int((r["want"] != r["finite"]).sum()) >= 10 * 32


@pytest.mark.parametrize("off,cap", _OFF_CAP)
def test_non_finite_encode(off, cap):
    """All six code-producing entry points: a block with a NaN or an
    infinity (NaN at element 0, 15, 16, 31, +Inf, -Inf, NaN beside Inf, NaN
    as the last element of a partial block; in a finish also from the packed
    input and from a finite sum that overflows) is byte 0xFF and 32 codes
    0x7F, and every other byte is that of the finite run."""
    r = _nonfinite()
    n, nbytes = r["x"].numel(), r["want"].numel()
    what = f"off={off} cap={cap}"
    keep_b, src_bad = _f32_src(r["bad"], off)
    keep_x, src_x = _f32_src(r["x"], off)
    keep_a, acc_bad = _f32_src(model.pad_super(r["bad"]), off)
    keep_s, acc_sum = _f32_src(r["acc"], off)
    zero, packed_in, packed_bad = (_zeros_packed(nbytes), _dev_bytes(r["packed_in"]),
                                   _dev_bytes(r["want"]))

    def outs(k):
        return [_guarded_bytes(nbytes) for _ in range(k)]

    def check(pairs, expects, kern):
        for (whole, out), expect in zip(pairs, expects):
            assert _guards_intact(whole, nbytes), (kern, what)
            _assert_bytes(out, expect, f"{kern} {what}")

    o = outs(2)
    _core.k_mx_quantize(src_bad.data_ptr(), n, o[0][1].data_ptr(), grid_cap=cap)
    _core.k_mx_quantize(src_x.data_ptr(), n, o[1][1].data_ptr(), grid_cap=cap)
    check(o, (r["want"], r["finite"]), "quantize")

    o = outs(2)
    assert _core.k_batched_mx_quantize([(src_bad.data_ptr(), o[0][1].data_ptr(), n),
                                        (src_x.data_ptr(), o[1][1].data_ptr(), n)],
                                       tile_cap=cap) == 1
    check(o, (r["want"], r["finite"]), "batched quantize")

    finish_in = ((acc_bad.data_ptr(), zero.data_ptr()), (acc_sum.data_ptr(), packed_in.data_ptr()),
                 (0, packed_bad.data_ptr()))
    finish_want = (r["want"], r["sum_want"], r["again"])
    o = outs(3)
    for (a, p), (whole, out) in zip(finish_in, o):
        _core.k_mx_finish(a, p, out.data_ptr(), nbytes, grid_cap=cap)
    check(o, finish_want, "finish (acc non-finite; packed input and overflow; no acc)")

    o = outs(3)
    assert _core.k_batched_mx_finish([(a, p, out.data_ptr(), nbytes)
                                      for (a, p), (whole, out) in zip(finish_in, o)],
                                     tile_cap=cap) == 1
    check(o, finish_want, "batched finish (acc non-finite; packed input and overflow; no acc)")


@pytest.mark.parametrize("off,cap", _OFF_CAP)
def test_non_finite_decode(off, cap):
    """Scale byte 0xFF over codes 0x7F reads as NaN in all 32 places through
    every fp32-producing kernel, with no case of its own in them, and the
    other blocks decode to the finite run's bits."""
    r = _nonfinite()
    n = r["x"].numel()
    npad = model.pad_super(r["x"]).numel()
    byte, codes = model.unpack(r["want"])
    clean = model.dequantize(*model.unpack(r["finite"]), npad)
    nan_at = torch.zeros(npad // 32, 32, dtype=torch.bool)
    nan_at[r["blocks"]] = True
    nan_at = nan_at.reshape(-1)
    want = torch.where(nan_at, torch.full((), float("nan")), clean)
    assert model.same_bits_or_nan(model.dequantize(byte, codes, npad), want)
    p = _dev_bytes(r["want"])
    what = f"off={off} cap={cap}"
    for alpha in (1.0, 0.5):
        whole, dst = _guarded_f32(n, off)
        _core.k_mx_dequantize(p.data_ptr(), n, dst.data_ptr(), alpha=alpha, grid_cap=cap)
        assert _f32_guards_intact(whole, n, off), what
        assert model.same_bits_or_nan(dst, want[:n] * alpha), ("dequantize", alpha, what)
        whole, dst = _guarded_f32(n, off)
        assert _core.k_batched_mx_dequantize([(dst.data_ptr(), p.data_ptr(), n)], alpha=alpha,
                                             tile_cap=cap) == 1
        assert _f32_guards_intact(whole, n, off), what
        assert model.same_bits_or_nan(dst, want[:n] * alpha), ("batched dequantize", alpha, what)
    for batched in (False, True):
        whole, a = _guarded_f32(npad, off)
        for assign, expect in ((True, want), (False, want + want)):
            if batched:
                assert _core.k_batched_mx_accumulate([(a.data_ptr(), p.data_ptr(), 0, p.numel())],
                                                     assign, tile_cap=cap) == 1
            else:
                _core.k_mx_accumulate(a.data_ptr(), p.data_ptr(), p.numel(), assign, grid_cap=cap)
            assert _f32_guards_intact(whole, npad, off), what
            assert model.same_bits_or_nan(a, expect), ("accumulate", batched, assign, what)


# ------------------------------------------------------------- end to end

_SIZES = (1000, 37, 513)
_NAN_AT = 70  # rank 1, parameter 0, step 1: inside its block 2, elements 64..95


def _rank_grads(rank):
    return [_data(n, seed=500 + 10 * rank + i) for i, n in enumerate(_SIZES)]


def _nan_gradsync_worker_fn(ps_mod, rank):
    from ps_lite_amd.parallel.dp import PSGradSync

    server = ps_mod.KVServer(0)
    server.set_gpu_dense_handle(mode="reduce", dtype="mxfp8")
    ps_mod.barrier("worker", ps_mod.WORKER_GROUP)
    worker = ps_mod.KVWorker(0, 0)
    params = [torch.nn.Parameter(torch.zeros(n, device="cuda:0")) for n in _SIZES]
    sync = PSGradSync(ps_mod, worker, params, num_workers=2, device=0, compress="mxfp8")
    outs = []
    for step in range(2):
        grads = _rank_grads(rank)
        if step == 1 and rank == 1:
            grads[0][_NAN_AT] = float("nan")
        for p, g in zip(params, grads):
            p.grad = g.to("cuda:0")
        sync.allreduce()
        torch.cuda.synchronize()
        outs.append([p.grad.cpu().numpy() for p in params])
    return outs, server


def test_gradsync_mxfp8_nan_reaches_both_workers():
    """Two workers, PSGradSync(compress="mxfp8"). Step 0, finite: both hold
    D(Q(D(Qa) + D(Qb))) / 2. Step 1, one NaN in one worker's gradient: both
    hold NaN in that block of 32 and step 0's bits everywhere else."""
    results = launch_local(2, 2, _nan_gradsync_worker_fn, joint=True, devices={0: 0, 1: 0},
                           env_extra={"XPS_POOL_GB": 4}, timeout=300)
    grads = [_rank_grads(0), _rank_grads(1)]
    blk = slice(_NAN_AT // 32 * 32, _NAN_AT // 32 * 32 + 32)
    for rank in (0, 1):
        clean, dirty = ([torch.from_numpy(a) for a in step] for step in results[rank])
        for i, n in enumerate(_SIZES):
            two = model.roundtrip(grads[0][i]) + model.roundtrip(grads[1][i])
            want = model.dequantize(*model.quantize(two), n, alpha=0.5)
            assert torch.equal(clean[i].view(torch.int32), want.view(torch.int32)), (rank, i)
            if i:
                assert torch.equal(dirty[i].view(torch.int32), want.view(torch.int32)), (rank, i)
                continue
            assert bool(torch.isnan(dirty[0][blk]).all()), rank
            keep = torch.ones(n, dtype=torch.bool)
            keep[blk] = False
            assert torch.equal(dirty[0][keep].view(torch.int32), want[keep].view(torch.int32)), rank
            assert not bool(torch.isfinite(dirty[0]).all())  # what an isfinite check must see
