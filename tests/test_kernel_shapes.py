"""Shapes and edge values at which the sum, batched and sparse kernels of
csrc/kernels.hip can go wrong: capped grids so that a few KiB take every
grid-stride and tile loop several times, sub-vector tails, pointers off a
16 B boundary, segment boundaries mid-wave and mid-block, empty segments,
lists past kMaxBatch, every bf16 rounding case, and keys at and beyond
both ends of a sparse table.

Every buffer a kernel writes lies inside a larger one filled with 0xAB
(16 guard bytes before, 48 after; whole guard rows around a sparse table)
and is compared whole, every source is compared afterwards, and every
reference is computed on the CPU from the same bytes: a byte copy, one
IEEE fp32 add, `(a.float() + b.float()).to(bfloat16)`, plain indexing.
Float results are compared bit for bit; only where the reference is NaN
may the output be any NaN. All marked gpu; a few MiB at most, except the
bf16 rounding table (8 MiB per operand)."""
import functools
import os

import numpy as np
import pytest

import ps_lite_amd as ps
from ps_lite_amd.parallel import launch_local

pytestmark = pytest.mark.gpu

_GUARD = 0xAB
_LEAD, _TRAIL = 16, 48  # guard bytes around every destination range
_REM = [0, 1, 255, 256, 257]
_DEV = "cuda:0"


def _torch():
    import torch
    return torch


# ------------------------------------------------------------------ helpers

def _elem(op):
    """(element size, torch float dtype, same-size int dtype, canonical NaN) of an op."""
    torch = _torch()
    if op == "f32":
        return 4, torch.float32, torch.int32, 0x7FC00000
    if op == "bf16":
        return 2, torch.bfloat16, torch.int16, 0x7FC0
    return 1, None, None, None


def _canon(buf, spans, op):
    """Copy of the uint8 buffer `buf` in which every NaN element of the
    payload spans [(byte offset, byte length)] reads as one canonical NaN."""
    es, fdt, idt, nan = _elem(op)
    out = buf.clone()
    if fdt is None:
        return out
    for at, n in spans:
        pay = out[at:at + n].clone()  # offset 0: viewable as any dtype
        pay.view(idt)[pay.view(fdt).isnan()] = nan
        out[at:at + n] = pay
    return out


def _assert_same(got, expect, spans, op, what):
    """Bit-exact over the whole buffer (payload and guards); where the
    reference is NaN the output must be NaN, of either sign and any payload."""
    torch = _torch()
    g, e = _canon(got, spans, op), _canon(expect, spans, op)
    if not torch.equal(g, e):
        bad = (g != e).nonzero().flatten()
        at = int(bad[0])
        lo = max(0, at - 4)
        raise AssertionError("%s: %d bytes differ, first at byte %d of %d (spans %s): got %s want %s"
                             % (what, bad.numel(), at, g.numel(), spans[:4],
                                got[lo:at + 8].tolist(), expect[lo:at + 8].tolist()))


def _ref(op, a, b):
    """CPU reference on uint8 tensors a (dst before) and b (src): uint8 result."""
    torch = _torch()
    es, fdt, idt, nan = _elem(op)
    if op == "assign" or a.numel() == 0:
        return b.clone()
    if op == "f32":
        return (a.view(fdt) + b.view(fdt)).view(torch.uint8)
    return (a.view(fdt).float() + b.view(fdt).float()).to(fdt).view(torch.uint8)


_F32_PAIRS = None


def _f32_pairs():
    """(dst, src) pairs a reduction can meet and randn never draws."""
    global _F32_PAIRS
    if _F32_PAIRS is None:
        torch = _torch()
        inf, nan, big = float("inf"), float("nan"), 3.4028234663852886e38  # FLT_MAX
        pairs = [(0.0, -0.0), (-0.0, -0.0), (-0.0, 0.0), (0.0, 0.0), (inf, 1.0), (-inf, 1.0),
                 (1.0, inf), (inf, -inf), (-inf, inf), (inf, inf), (nan, 1.0), (1.0, nan),
                 (nan, nan), (big, big), (-big, -big), (big, -big), (1.5, -1.5),
                 (big, 1.0), (1.0, 2.0 ** -24), (1.0, 2.0 ** -23)]
        _F32_PAIRS = (torch.tensor([p[0] for p in pairs], dtype=torch.float32),
                      torch.tensor([p[1] for p in pairs], dtype=torch.float32))
    return _F32_PAIRS


def _operands(op, nbytes, seed):
    """(dst before, src) as uint8 CPU tensors of nbytes each."""
    torch = _torch()
    g = torch.Generator(device="cpu").manual_seed(seed)
    es, fdt, idt, nan = _elem(op)
    n = nbytes // es
    if op == "assign":
        return (torch.full((nbytes,), _GUARD, dtype=torch.uint8),
                torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=g))
    if n == 0:
        return torch.empty(0, dtype=torch.uint8), torch.empty(0, dtype=torch.uint8)
    if op == "f32":
        a = torch.randn(n, generator=g)
        b = torch.randn(n, generator=g)
        pa, pb = _f32_pairs()
        at = torch.arange(3 % n, n, 7)  # every 7th element: vector body and tail alike
        a[at] = pa[torch.arange(at.numel()) % pa.numel()]
        b[at] = pb[torch.arange(at.numel()) % pb.numel()]
        at = torch.arange(5 % n, n, 11)  # pairs that cancel exactly
        b[at] = -a[at]
    else:
        a = torch.randn(n, generator=g).to(fdt)
        b = (torch.randn(n, generator=g) * 0.37).to(fdt)
        at = torch.arange(2 % n, n, 5)  # every 5th element: any bit pattern at all
        for t in (a, b):
            t.view(idt)[at] = torch.randint(-32768, 32768, (at.numel(),), dtype=idt, generator=g)
    return a.view(torch.uint8).clone(), b.view(torch.uint8).clone()


def _guarded(payload, lead=_LEAD):
    """CPU uint8 buffer: lead guard bytes, the payload, 48 guard bytes."""
    torch = _torch()
    n = payload.numel()
    host = torch.full((lead + n + _TRAIL,), _GUARD, dtype=torch.uint8)
    host[lead:lead + n] = payload
    return host


def _to_dev(host):
    d = host.to(_DEV)
    assert d.data_ptr() % 16 == 0
    return d


# ------------------------------------------------- dense assign and sums

def _k_dense(op, dptr, sptr, nbytes, grid_cap):
    es = _elem(op)[0]
    fn = {"assign": ps._core.k_dense_assign, "f32": ps._core.k_dense_sum_f32,
          "bf16": ps._core.k_dense_sum_bf16}[op]
    fn(dptr, sptr, nbytes // es, grid_cap=grid_cap)


def _dense(op, nbytes, grid_cap, dskew=0, sskew=0, operands=None):
    """One launch on a destination `dskew` bytes and a source `sskew` bytes
    off a 16 B boundary."""
    a, b = operands if operands is not None else _operands(op, nbytes, nbytes * 3 + grid_cap)
    lead = _LEAD + dskew
    expect = _guarded(_ref(op, a, b), lead)
    dst_d = _to_dev(_guarded(a, lead))
    src = _guarded(b, lead=sskew)
    src_d = _to_dev(src)
    _k_dense(op, dst_d.data_ptr() + lead, src_d.data_ptr() + sskew, nbytes, grid_cap)
    _assert_same(dst_d.cpu(), expect, [(lead, nbytes)], op,
                 "%s nbytes=%d cap=%d skew=%d/%d" % (op, nbytes, grid_cap, dskew, sskew))
    assert _torch().equal(src_d.cpu(), src), "source changed"


_CAPS = [1, 2, 0]
# every tail length of the op, every remainder of the 256-lane block
_ASSIGN_SIZES = ([16 * (2048 + r) for r in _REM] +
                 [16 * (2048 + _REM[t % 5]) + t for t in range(1, 16)])
_F32_SIZES = [16 * (2048 + r) + 4 * t for r in _REM for t in (1, 2, 3)]
_BF16_SIZES = [16 * (2048 + _REM[t % 5]) + 2 * t for t in range(1, 8)]


@pytest.mark.parametrize("grid_cap", _CAPS)
@pytest.mark.parametrize("nbytes", _ASSIGN_SIZES)
def test_dense_assign_shapes(nbytes, grid_cap):
    _dense("assign", nbytes, grid_cap)


@pytest.mark.parametrize("grid_cap", _CAPS)
@pytest.mark.parametrize("nbytes", _F32_SIZES)
def test_dense_sum_f32_shapes(nbytes, grid_cap):
    _dense("f32", nbytes, grid_cap)


@pytest.mark.parametrize("grid_cap", _CAPS)
@pytest.mark.parametrize("nbytes", _BF16_SIZES)
def test_dense_sum_bf16_shapes(nbytes, grid_cap):
    _dense("bf16", nbytes, grid_cap)


@pytest.mark.parametrize("op,nbytes", [("assign", 0), ("assign", 3), ("assign", 15),
                                       ("f32", 0), ("f32", 4), ("f32", 12),
                                       ("bf16", 0), ("bf16", 2), ("bf16", 6), ("bf16", 14)])
def test_dense_below_one_vector(op, nbytes):
    for cap in (0, 1):
        _dense(op, nbytes, cap)


_SKEWS = [(0, 1), (1, 0), (1, 1)]  # (destination, source) in units of the skew


@pytest.mark.parametrize("grid_cap", [0, 1])
@pytest.mark.parametrize("dskew,sskew", _SKEWS)
@pytest.mark.parametrize("op,skew,nbytes", [("assign", 4, 16 * 2049 + 7),
                                            ("f32", 4, 16 * 2049 + 12),
                                            ("bf16", 2, 16 * 2049 + 10)])
def test_dense_skewed_pointers_take_element_loop(op, skew, nbytes, dskew, sskew, grid_cap):
    _dense(op, nbytes, grid_cap, dskew * skew, sskew * skew)


@pytest.mark.parametrize("grid_cap", _CAPS)
def test_dense_sum_f32_subnormals_not_flushed_to_zero(grid_cap):
    """Subnormal inputs, and normal inputs whose sum is subnormal: a build
    that flushed fp32 denormals to zero would differ from the CPU add."""
    torch = _torch()
    g = torch.Generator(device="cpu").manual_seed(950 + grid_cap)
    n = 4 * (2048 + 257) + 3
    half = n // 2
    sign = lambda k: torch.randint(0, 2, (k,), dtype=torch.int64, generator=g) << 31
    # subnormal + subnormal: subnormal, or just normal
    a1 = torch.randint(1, 1 << 23, (half,), dtype=torch.int64, generator=g) | sign(half)
    b1 = torch.randint(1, 1 << 23, (half,), dtype=torch.int64, generator=g) | sign(half)
    # two numbers of the lowest normal binade, opposite signs: the sum is subnormal or zero
    a2 = torch.randint(1 << 23, 1 << 24, (n - half,), dtype=torch.int64, generator=g)
    b2 = torch.randint(1 << 23, 1 << 24, (n - half,), dtype=torch.int64, generator=g) | (1 << 31)
    bits = lambda x: (x - ((x >> 31) << 32)).to(torch.int32)  # two's complement of bit 31
    a = bits(torch.cat([a1, a2])).view(torch.float32)
    b = bits(torch.cat([b1, b2])).view(torch.float32)
    tiny = torch.finfo(torch.float32).tiny
    want = a + b
    # the reference itself keeps them, or the case would prove nothing
    assert int(((want.abs() < tiny) & (want != 0)).sum()) > n // 2
    assert int((a.abs() < tiny).sum()) == half
    _dense("f32", 4 * n, grid_cap,
           operands=(a.view(torch.uint8).clone(), b.view(torch.uint8).clone()))


# ------------------------------------------------------ bf16 rounding table

_BF16_NAMED = [0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x0080, 0x3F80, 0xBF80, 0x3B80, 0x3C00,
               0x3F81, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0, 0x7F81, 0xFFFF, 0x7700, 0x3380]


@functools.lru_cache(maxsize=None)
def _bf16_table():
    """(dst before, src, reference) as uint8: all 65536 dst patterns against
    64 src patterns, 4 Mi sums. Computed once, shared, never modified."""
    torch = _torch()
    g = torch.Generator(device="cpu").manual_seed(0xBF16)
    drawn = torch.randint(0, 65536, (44,), generator=g).tolist()
    pats = torch.tensor(_BF16_NAMED + drawn, dtype=torch.int32)
    assert pats.numel() == 64

    def as_bf16(x):  # int32 patterns 0..65535 -> bf16 with those bits
        return (x - ((x >> 15) << 16)).to(torch.int16).view(torch.bfloat16)

    a = as_bf16(torch.arange(65536, dtype=torch.int32).repeat(64))
    b = as_bf16(pats.repeat_interleave(65536))
    want = (a.float() + b.float()).to(torch.bfloat16)

    def at(dst, src):
        return int(want.view(torch.int16)[_BF16_NAMED.index(src) * 65536 + dst]) & 0xFFFF

    # what the table is for is really in it
    assert at(0x3F80, 0x3B80) == 0x3F80 and at(0x3F81, 0x3B80) == 0x3F82  # ties go to even
    # max + half an ulp: the mantissa carries into the exponent and reaches infinity
    assert at(0x7B00, 0x7F7F) == 0x7F80
    assert at(0x7700, 0x7F7F) == 0x7F7F  # 2^111 is far below that half ulp (2^119)
    assert at(0x0001, 0x0001) == 0x0002 and at(0x007F, 0x0001) == 0x0080  # subnormal sums
    nan = want.isnan()
    # three of the 64 partners are NaN themselves, and so are 254 of the dst patterns
    assert float(nan.float().mean()) > 3 / 64
    assert at(0x7F80, 0xFF80) & 0x7FFF > 0x7F80  # inf + -inf is a NaN
    return tuple(t.view(torch.uint8).clone() for t in (a, b, want))


def _bf16_table_run(launch):
    a, b, want = _bf16_table()
    n = a.numel()
    expect = _guarded(want)
    dst_d = _to_dev(_guarded(a))
    src_d = _to_dev(b)
    launch(dst_d.data_ptr() + _LEAD, src_d.data_ptr(), n)
    _assert_same(dst_d.cpu(), expect, [(_LEAD, n)], "bf16", "bf16 table")
    assert _torch().equal(src_d.cpu(), b), "source changed"


def test_dense_sum_bf16_rounding_table():
    _bf16_table_run(lambda d, s, n: ps._core.k_dense_sum_bf16(d, s, n // 2))


def test_batched_sum_bf16_rounding_table():
    _bf16_table_run(lambda d, s, n: ps._core.k_batched_sum_bf16([(d, s, n)]))


# --------------------------------------------------------------- batched

_BOUNDARY = [16 * 257, 16 * 255, 16, 16 * 513]  # boundaries mid-wave and mid-block
_BATCHED_CASES = (
    [("boundary_cap%d" % c, _BOUNDARY, c) for c in (1, 2, 3, 0)] +
    [("many16", [16] * 64, 0),
     ("split130", [16] * 130, 0)] +  # three launches, the last of two segments
    [("rem%d" % r, [16 * (2048 + r)], 0) for r in _REM] +
    [("rem%d_then48" % r, [16 * (2048 + r), 48], 0) for r in _REM] +
    [("zeros_mixed", [0, 16 * 300, 0, 0, 48, 16 * 257, 0], 0),
     ("zeros_mixed_cap2", [0, 16 * 300, 0, 0, 48, 16 * 257, 0], 2),
     ("zeros_around_split", [0] * 63 + [16 * 5] + [0] * 64 + [32, 0], 0),
     ("all_zero", [0, 0, 0], 0),
     ("all_zero_cap1", [0] * 70, 1),
     ("short_last_cap5", [16 * 1000, 16 * 1000, 16 * 1001], 5)]
)
_BATCHED_OPS = ["assign", "f32", "bf16"]
_BATCHED_IDS = ["%s-%s" % (op, c[0]) for op in _BATCHED_OPS for c in _BATCHED_CASES]
_BATCHED_PARAMS = [(op,) + c for op in _BATCHED_OPS for c in _BATCHED_CASES]


def _batched(ps_mod, op, name, sizes, tile_cap):
    """One k_batched_* call over `sizes`; every destination in its own
    guarded slot of one buffer, slots in shuffled address order."""
    torch = _torch()
    seed = sum(sizes) * 7 + len(sizes) * 131 + tile_cap
    total = sum(sizes)
    a, b = _operands(op, total, seed)
    want = _ref(op, a, b)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    order = torch.randperm(len(sizes), generator=g).tolist()  # order[k]: segment in slot k
    if order == sorted(order):
        order.reverse()  # never address order (a single segment aside)
    slot_at, at = {}, 0
    for seg in order:
        slot_at[seg] = at + _LEAD
        at += _LEAD + sizes[seg] + _TRAIL
    # `total` more guard bytes behind the slots and behind the sources: a
    # kernel that takes a chunk for the wrong segment addresses less than
    # `total` bytes past that segment's start, which is still inside
    span = at + total
    expect = torch.full((span,), _GUARD, dtype=torch.uint8)
    start = torch.full((span,), _GUARD, dtype=torch.uint8)
    s_at, spans = 0, []
    for seg, n in enumerate(sizes):
        d = slot_at[seg]
        start[d:d + n] = a[s_at:s_at + n]
        expect[d:d + n] = want[s_at:s_at + n]
        spans.append((d, n))
        s_at += n
    dst_d = _to_dev(start)
    src = torch.cat([b, torch.full((total + 16,), _GUARD, dtype=torch.uint8)])
    src_d = _to_dev(src)
    segs, s_at = [], 0
    for seg, n in enumerate(sizes):
        segs.append((dst_d.data_ptr() + slot_at[seg], src_d.data_ptr() + s_at, n))
        s_at += n
    fn = {"assign": ps_mod._core.k_batched_assign, "f32": ps_mod._core.k_batched_sum_f32,
          "bf16": ps_mod._core.k_batched_sum_bf16}[op]
    fn(segs, tile_cap)
    _assert_same(dst_d.cpu(), expect, spans, op, "batched %s %s" % (op, name))
    assert torch.equal(src_d.cpu(), src), "source changed"


@pytest.mark.parametrize("op,name,sizes,tile_cap", _BATCHED_PARAMS, ids=_BATCHED_IDS)
def test_batched_shapes(op, name, sizes, tile_cap):
    assert os.environ.get("XPS_BALANCED_BATCH", "1") != "0"  # the balanced kernel is under test
    _batched(ps, op, name, sizes, tile_cap)


def test_batched_rejects_misaligned_segment():
    torch = _torch()
    d = torch.zeros(64, dtype=torch.uint8, device=_DEV)
    s = torch.zeros(64, dtype=torch.uint8, device=_DEV)
    for fn in (ps._core.k_batched_assign, ps._core.k_batched_sum_f32,
               ps._core.k_batched_sum_bf16):
        for seg in [(d.data_ptr() + 4, s.data_ptr(), 16), (d.data_ptr(), s.data_ptr() + 8, 16),
                    (d.data_ptr(), s.data_ptr(), 24)]:
            with pytest.raises(ValueError):
                fn([seg])
    assert int(d.cpu().sum()) == 0


def _legacy_child_fn(ps_mod, rank):
    """Runs in a fresh process with XPS_BALANCED_BATCH=0 (read once per
    process): every batched case, one result each."""
    import traceback

    out = {"env": os.environ.get("XPS_BALANCED_BATCH")}
    for cid, (op, name, sizes, tile_cap) in zip(_BATCHED_IDS, _BATCHED_PARAMS):
        try:
            _batched(ps_mod, op, name, sizes, tile_cap)
            out[cid] = "ok"
        except AssertionError:
            out[cid] = traceback.format_exc(limit=2)
    return out


@functools.lru_cache(maxsize=None)
def _legacy_results():
    results = launch_local(1, 1, _legacy_child_fn, joint=True, devices={0: 0},
                           env_extra={"XPS_POOL_GB": 4, "XPS_BALANCED_BATCH": 0}, timeout=300)
    return results[0]


@pytest.mark.parametrize("cid", _BATCHED_IDS)
def test_batched_shapes_legacy_kernels_in_child(cid):
    """The same cases through batched_legacy_kernel (XPS_BALANCED_BATCH=0):
    one child process for all of them, started by the first case."""
    res = _legacy_results()
    assert res["env"] == "0"
    assert res[cid] == "ok", res[cid]


# ----------------------------------------------------------------- sparse

_ROWS = 64  # table rows, between whole guard rows
_ROW_LENS = [1, 3, 4, 5, 64, 68, 258, 260]  # 258: two steps of the in-row loop
_NROWS = [1, 257, 1000]
_KEYING = [(0, 0), (16, 5), (48, 5)]  # (key_shift, row_base)
_U64 = (1 << 64) - 1


def _encode(rng, row, shift, base):
    """Key of local row `row` (may be out of range, or negative down to
    -base), random junk in the bits below the shift."""
    junk = int(rng.integers(0, 1 << shift)) if shift else 0
    return ((row + base) << shift) | junk


def _edge_keys(rng, shift, base):
    """[(key, local row or -1)]: one below row_base (the subtraction wraps),
    exactly table_rows, table_rows - 1, and 2^64 - 1."""
    out = [(_encode(rng, _ROWS, shift, base), -1), (_encode(rng, _ROWS - 1, shift, base), _ROWS - 1),
           (_U64, -1)]
    if base:
        out.append((_encode(rng, -1, shift, base), -1))
    return out


def _outside(rng, shift, base):
    kind = int(rng.integers(0, 4))
    if kind == 0 and base:
        return _encode(rng, -1 - int(rng.integers(0, base)), shift, base)
    if kind == 1:
        return _U64
    return _encode(rng, _ROWS + int(rng.integers(0, 1000)), shift, base)


def _key_list(rng, nrows, shift, base, unique):
    """(keys uint64[nrows], local int64[nrows], -1 where out of range). With
    `unique` no in-range row repeats (the rest of the list is out of range)."""
    edges = _edge_keys(rng, shift, base)
    if nrows < 8:
        raise ValueError("short lists are built by the caller")
    pairs = list(edges)
    used = {_ROWS - 1}
    pool = [r for r in rng.permutation(_ROWS).tolist() if r not in used]
    while len(pairs) < nrows:
        if unique:
            if pool and rng.random() < 0.5:
                r = pool.pop()
                pairs.append((_encode(rng, r, shift, base), r))
            else:
                pairs.append((_outside(rng, shift, base), -1))
        elif rng.random() < 0.9:
            r = int(rng.integers(0, _ROWS))
            pairs.append((_encode(rng, r, shift, base), r))
        else:
            pairs.append((_outside(rng, shift, base), -1))
    perm = rng.permutation(nrows)
    keys = np.array([pairs[i][0] for i in perm], dtype=np.uint64)
    local = np.array([pairs[i][1] for i in perm], dtype=np.int64)
    return keys, local


def _key_lists(rng, nrows, shift, base, unique):
    """The lists to run for one (nrows, keying): one list, or for a single
    row one list per edge key and one ordinary row."""
    if nrows >= 8:
        return [_key_list(rng, nrows, shift, base, unique)]
    singles = _edge_keys(rng, shift, base) + [(_encode(rng, 17, shift, base), 17)]
    return [(np.array([k], dtype=np.uint64), np.array([r], dtype=np.int64)) for k, r in singles]


def _table_bytes(row_len):
    """(lead, table bytes): two whole guard rows on each side, the lead
    rounded up to 16 bytes so that the table itself is 16 B-aligned."""
    lead = -(-(2 * row_len * 4) // 16) * 16
    return lead, _ROWS * row_len * 4


def _np_dev(arr):
    """numpy array -> uint8 device tensor with the same bytes."""
    torch = _torch()
    d = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).to(_DEV)
    assert d.data_ptr() % 16 == 0
    return d


def _dev_np(t, dtype):
    return t.cpu().numpy().view(dtype)


def _embed_table(table, row_len):
    """float32 [64, row_len] -> (host uint8 array with guards, lead)."""
    lead, nb = _table_bytes(row_len)
    host = np.full(lead + nb + lead, _GUARD, dtype=np.uint8)
    host[lead:lead + nb] = table.reshape(-1).view(np.uint8)
    return host, lead


def _sparse_combos():
    for cap in (1, 0):
        for shift, base in _KEYING:
            yield cap, shift, base


@pytest.mark.parametrize("nrows", _NROWS)
@pytest.mark.parametrize("row_len", _ROW_LENS)
def test_sparse_gather_shapes(row_len, nrows):
    rng = np.random.default_rng(row_len * 1009 + nrows)
    # any bit pattern: a gather only moves bytes
    table = rng.integers(0, 1 << 32, (_ROWS, row_len), dtype=np.uint64).astype(np.uint32)
    host, lead = _embed_table(table, row_len)
    tab_d = _np_dev(host)
    for cap, shift, base in _sparse_combos():
        for keys, local in _key_lists(rng, nrows, shift, base, unique=False):
            n = keys.size
            want = np.where((local >= 0)[:, None], table[np.maximum(local, 0)], np.uint32(0))
            expect = np.full(_LEAD + n * row_len * 4 + _TRAIL, _GUARD, dtype=np.uint8)
            expect[_LEAD:_LEAD + n * row_len * 4] = want.astype(np.uint32).reshape(-1).view(np.uint8)
            out_d = _np_dev(np.full(expect.size, _GUARD, dtype=np.uint8))
            keys_d = _np_dev(keys)
            ps._core.k_sparse_gather_f32(tab_d.data_ptr() + lead, keys_d.data_ptr(), n, row_len,
                                         out_d.data_ptr() + _LEAD, key_shift=shift,
                                         row_base=base, table_rows=_ROWS, grid_cap=cap)
            what = (row_len, nrows, cap, shift, base)
            assert np.array_equal(_dev_np(out_d, np.uint8), expect), what
            assert np.array_equal(_dev_np(tab_d, np.uint8), host), what
            assert np.array_equal(_dev_np(keys_d, np.uint64), keys), what


def _scatter(row_len, nrows, add):
    rng = np.random.default_rng(row_len * 2003 + nrows * 3 + int(add))
    for cap, shift, base in _sparse_combos():
        for keys, local in _key_lists(rng, nrows, shift, base, unique=True):
            n = keys.size
            if add:
                table = rng.standard_normal((_ROWS, row_len)).astype(np.float32)
                src = rng.standard_normal((n, row_len)).astype(np.float32)
            else:  # any bit pattern: an assign only moves bytes
                table = rng.integers(0, 1 << 32, (_ROWS, row_len),
                                     dtype=np.uint64).astype(np.uint32).view(np.float32)
                src = rng.integers(0, 1 << 32, (n, row_len),
                                   dtype=np.uint64).astype(np.uint32).view(np.float32)
            host, lead = _embed_table(table, row_len)
            want = table.copy()
            inside = local >= 0
            assert np.unique(local[inside]).size == int(inside.sum())
            if add:
                want[local[inside]] = want[local[inside]] + src[inside]  # one fp32 add each
            else:
                want[local[inside]] = src[inside]
            expect, _ = _embed_table(want, row_len)
            tab_d, src_d, keys_d = _np_dev(host), _np_dev(src), _np_dev(keys)
            args = (tab_d.data_ptr() + lead, keys_d.data_ptr(), n, row_len, src_d.data_ptr())
            kw = dict(key_shift=shift, row_base=base, table_rows=_ROWS, grid_cap=cap)
            if add:
                ps._core.k_sparse_scatter_add_f32(*args, False, **kw)
            else:
                ps._core.k_sparse_scatter_assign_f32(*args, **kw)
            what = (row_len, nrows, cap, shift, base)
            assert np.array_equal(_dev_np(tab_d, np.uint8), expect), what
            assert np.array_equal(_dev_np(src_d, np.uint8), src.reshape(-1).view(np.uint8)), what
            assert np.array_equal(_dev_np(keys_d, np.uint64), keys), what


@pytest.mark.parametrize("nrows", _NROWS)
@pytest.mark.parametrize("row_len", _ROW_LENS)
def test_sparse_scatter_assign_unique_rows(row_len, nrows):
    _scatter(row_len, nrows, add=False)


@pytest.mark.parametrize("nrows", _NROWS)
@pytest.mark.parametrize("row_len", _ROW_LENS)
def test_sparse_scatter_add_unique_rows(row_len, nrows):
    _scatter(row_len, nrows, add=True)


@pytest.mark.parametrize("row_len,atomic", [(3, True), (3, False), (64, True), (258, False)])
def test_sparse_scatter_add_duplicate_rows(row_len, atomic):
    """1000 updates onto 7 rows. Integers in [-1024, 1024] on an integer
    table: every partial sum is exact in fp32 in any order, so the result is
    bit-exact although the order of the atomic adds is not fixed. A row_len
    that is no multiple of 4 takes the atomic kernel whatever `atomic` says."""
    rng = np.random.default_rng(row_len * 7 + int(atomic))
    nrows = 1000
    hot = rng.permutation(_ROWS - 1)[:7]  # table_rows - 1 comes with the edge keys
    for cap, shift, base in _sparse_combos():
        edges = _edge_keys(rng, shift, base)
        local = np.concatenate([hot[rng.integers(0, 7, nrows - len(edges))],
                                np.array([e[1] for e in edges], dtype=np.int64)])
        keys = np.array([_encode(rng, int(r), shift, base) for r in local[:nrows - len(edges)]] +
                        [e[0] for e in edges], dtype=np.uint64)
        perm = rng.permutation(nrows)
        local, keys = local[perm], keys[perm]
        table = rng.integers(-1024, 1025, (_ROWS, row_len)).astype(np.float32)
        src = rng.integers(-1024, 1025, (nrows, row_len)).astype(np.float32)
        inside = local >= 0
        assert np.unique(local[inside]).size == 8  # the 7 rows and table_rows - 1
        want = table.copy()
        np.add.at(want, local[inside], src[inside])
        host, lead = _embed_table(table, row_len)
        expect, _ = _embed_table(want, row_len)
        tab_d, src_d, keys_d = _np_dev(host), _np_dev(src), _np_dev(keys)
        ps._core.k_sparse_scatter_add_f32(tab_d.data_ptr() + lead, keys_d.data_ptr(), nrows,
                                          row_len, src_d.data_ptr(), atomic, key_shift=shift,
                                          row_base=base, table_rows=_ROWS, grid_cap=cap)
        what = (row_len, atomic, cap, shift, base)
        assert np.array_equal(_dev_np(tab_d, np.uint8), expect), what
        assert np.array_equal(_dev_np(src_d, np.uint8), src.reshape(-1).view(np.uint8)), what
        assert np.array_equal(_dev_np(keys_d, np.uint64), keys), what
