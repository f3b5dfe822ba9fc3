"""The bf16-table kernels (csrc/sparse_table.hip) against tests/bf16_store_model.py, bit for bit:
every assertion on table, state and out is an equality of bits. test_sparse_bf16.py bounds a stored
value within an ulp; here the stored bits are the model's R(x), with the 16 random bits of every
element computed from (seed, local table row, element index).

x is exact where the arithmetic is: an assign has none, an add is one IEEE fp32 add (numpy's), and
a step is exact on inputs no contraction can change. hipcc may fuse a * b + c, which differs from
the unfused form only where a * b is inexact, so the steps run on gradients k / 16 with |k| <= 64
(squares and sums of up to 2056 of them are exact fp32), beta1 = beta2 = 1/2, p = 2^-k and bf16
weights, with lr, eps and the state arbitrary; division and square root round correctly. On those
inputs the fp32 kernels of sparse_table.hip leave the same x and state bits as the model (the claim
of sparse_elem.h), and on ordinary inputs the element-wise bf16 kernels leave the fp32 kernels'
state bits and R of their x.

Row lengths by the element index they reach: 4, 12, 20 and 130 on the element path (a word
recomputed per element), 197 there with lanes 0 to 4 streaming twice, 8 / 24 / 72 resident on the
8-element path, 1032 one streaming unit, 1544 the first row whose lane 0 streams twice, 2056, and
64 / 1032 with the table 2 bytes off (the element path on a vector-shaped row)."""
import itertools

import numpy as np
import pytest

import bf16_store_model as model
import ps_lite_amd as ps
from test_sparse_adagrad import _ROWS, _Dev, _keys
from test_sparse_lazy_adam import _B1, _B2, _EPS, _LR, fresh

pytestmark = pytest.mark.gpu

_LOWS = [0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF]
# an even and an odd high half, both signs; then +-0, +-Inf, the two largest finite values' upper
# halves (they round to Inf) and the carry into the exponent
_FINITE = [h << 16 | low for h in (0x3F80, 0x3F81, 0xBF80, 0xBF81) for low in _LOWS] + [
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7F8000, 0x7F7FFFFF, 0x3FFFFFFF]
# fp32 subnormals, and the bf16 subnormals 0x0001 and 0x807F widened
_SUBNORMAL = [0x00000001, 0x00007FFF, 0x00008000, 0x0000FFFF, 0x007FFFFF, 0x80008001, 0x00010000,
              0x807F0000]
_NAN = [0x7FC00000, 0x7F800001, 0x7F80FFFF, 0xFFC12345, 0x7F810000]
_SEEDS = [0, 3, 2 ** 64 - 1]  # the last wraps seed + (row + 1) * phi


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same(got, want, what):
    """bit equality of two arrays of one itemsize, with the first difference in the message"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, what
    kind = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    g, w = got.view(kind), want.view(kind)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        at = tuple(bad[0])
        raise AssertionError("%s: %d of %d differ, first at %s: got %#x want %#x"
                             % (what, len(bad), g.size, at, g[at], w[at]))


def _bits_of(x):
    """the bf16 bits of fp32 values that are bf16"""
    u = _u32(x)
    assert not (u & 0xFFFF).any()
    return (u >> 16).astype(np.uint16)


def _fields(rounding, seed, rows, row_len):
    return model.r16(seed, rows, row_len) if rounding == "stochastic" else None


def _is_nan_bits(b):
    return ((b & 0x7F80) == 0x7F80) & ((b & 0x7F) != 0)


# ------------------------------------------------------------ (a) assign and gather, no arithmetic

@pytest.mark.parametrize("row_len,grid_cap,skew", [(1, 1, 0), (3, 0, 0), (8, 1, 0), (72, 0, 0), (64, 0, 2)])
def test_assign_and_gather_edge_table(row_len, grid_cap, skew):
    rng = np.random.default_rng([row_len, grid_cap, skew])
    keys, local = _keys(rng, 257, 0, 0)
    inside, rows = local >= 0, local[local >= 0]
    pool = np.array(_FINITE + _SUBNORMAL + _NAN, dtype=np.uint32)
    n = len(rows) * row_len
    kw = dict(table_rows=_ROWS, grid_cap=grid_cap)
    for start in range(0, len(pool), n):  # until every pattern has been a source
        src = rng.standard_normal((257, row_len)).astype(np.float32)
        _u32(src)[inside] = np.roll(pool, -start)[np.arange(n) % len(pool)].reshape(-1, row_len)
        before = model.store(rng.standard_normal((_ROWS, row_len)).astype(np.float32))
        tab_d, src_d, keys_d = _Dev(before, skew), _Dev(src), _Dev(keys)
        out_d = _Dev(np.full((257, row_len), np.nan, dtype=np.float32))
        out16_d = _Dev(np.full((257, row_len), 0xABAB, dtype=np.uint16))
        ps._core.k_sparse_scatter_assign_bf16(tab_d.ptr, keys_d.ptr, 257, row_len, src_d.ptr, **kw)
        ps._core.k_sparse_gather_bf16(tab_d.ptr, keys_d.ptr, 257, row_len, out_d.ptr, **kw)
        ps._core.k_sparse_gather_bf16_wire(tab_d.ptr, keys_d.ptr, 257, row_len, out16_d.ptr, **kw)
        want = before.copy()
        want[rows] = model.store(src[inside])
        got = tab_d.read()
        _same(got, want, "table")
        # every NaN source is a stored NaN (none became Inf) and nothing else is one
        assert np.array_equal(_is_nan_bits(got[rows]), np.isnan(src[inside]))
        assert np.array_equal(np.isnan(model.widen(got[rows])), np.isnan(src[inside]))
        there = want[np.maximum(local, 0)]
        _same(out_d.read(), np.where(inside[:, None], _u32(model.widen(there)), 0).astype(np.uint32),
              "fp32 gather")
        _same(out16_d.read(), np.where(inside[:, None], there, 0).astype(np.uint16), "bf16 gather")
        _same(src_d.read(), src, "src")
        assert np.array_equal(keys_d.read(), keys)


# ------------------------------------------------------------------------- (b) the add, one fp32 add

# (row_len, skew, wire, rounding, seed, key_shift, row_base, grid_cap): every row length with both
# wires and both roundings; the seeds, the shifted keys and grid_cap take turns
_ADD_CASES = [(L, skew, wire, rounding, _SEEDS[(i + j) % 3]) + ((48, 5) if (i + j) % 3 == 1 else (0, 0))
              + ((i + j) & 1,)
              for i, (L, skew) in enumerate([(4, 0), (12, 0), (20, 0), (8, 0), (72, 0), (1032, 0),
                                             (1544, 0), (64, 2)])
              for j, (wire, rounding) in enumerate(itertools.product(["f32", "bf16"],
                                                                     ["stochastic", "nearest"]))]
# (table bits, source bits): +0 plus every finite edge pattern (-0.0 onto +0 gives +0); the largest
# finite bf16 plus 2^119, whose sum 0x7F7F8000 lies half way to Inf; negative sums that are exact,
# a tie at an odd high half that carries into the exponent, and just past it
_PLANTED = [(0x0000, u) for u in _FINITE] + [
    (0x7F7F, 0x7B000000), (0xBFFF, 0xBC000000), (0xBFFF, 0xBB800000), (0xBFFF, 0xBB800001),
    (0xC000, 0xB0000000), (0xBF80, 0xBF800000)]


def _add_message(rng, row_len, wire, shift, base):
    """(keys, local, table bits, fp32 src): random normals with _PLANTED spread over the rows of
    the message that lie in the table; a bf16 wire carries the upper halves"""
    keys, local = _keys(rng, 257, shift, base)
    ins = np.flatnonzero(local >= 0)
    tab = model.store(rng.standard_normal((_ROWS, row_len)).astype(np.float32))
    src = rng.standard_normal((257, row_len)).astype(np.float32)
    if wire == "bf16":
        src = model.widen(model.store(src))
    for (wb, su), at in zip(_PLANTED, rng.choice(len(ins) * row_len, len(_PLANTED), replace=False)):
        r, e = divmod(int(at), row_len)
        tab[local[ins[r]], e] = wb
        _u32(src)[ins[r], e] = su & 0xFFFF0000 if wire == "bf16" else su
    return keys, local, tab, src


def _add(wire, tab, skew, keys, src, **kw):
    tab_d, keys_d = _Dev(tab, skew), _Dev(keys)
    src_d = _Dev(_bits_of(src) if wire == "bf16" else src)
    fn = ps._core.k_sparse_scatter_add_bf16_wire if wire == "bf16" else ps._core.k_sparse_scatter_add_bf16
    fn(tab_d.ptr, keys_d.ptr, len(keys), src.shape[1], src_d.ptr, table_rows=_ROWS, **kw)
    _same(src_d.read(), src_d.src, "src")
    assert np.array_equal(keys_d.read(), keys)
    return tab_d.read()


def _add_model(tab, local, src, rounding, seed):
    inside, rows = local >= 0, local[local >= 0]
    total = model.widen(tab[rows]) + src[inside]  # numpy's float32 add is the kernel's IEEE add
    want = tab.copy()
    want[rows] = model.store(total, _fields(rounding, seed, rows, src.shape[1]))
    return want, total


@pytest.mark.parametrize("row_len,skew,wire,rounding,seed,shift,base,grid_cap", _ADD_CASES)
def test_add_exact(row_len, skew, wire, rounding, seed, shift, base, grid_cap):
    rng = np.random.default_rng([row_len, skew, len(wire), len(rounding), shift])
    keys, local, tab, src = _add_message(rng, row_len, wire, shift, base)
    want, total = _add_model(tab, local, src, rounding, seed)
    u = _u32(total)
    assert (u == 0x7F7F8000).any() and (u == 0xBFFF8000).any() and (u == 0xC0000000).any()
    assert not np.isnan(total).any() and ((u & 0xFFFF) != 0).mean() > 0.4  # many sums do round
    assert (u == 0).any() and not (u == 0x80000000).any()  # -0.0 onto +0
    if wire == "f32":
        assert (u == 0x3FFFFFFF).any() and (u == 0xBF81FFFF).any()
    got = _add(wire, tab, skew, keys, src, rounding=rounding, seed=seed, key_shift=shift,
               row_base=base, grid_cap=grid_cap)
    # rows outside the message and keys outside the table: want holds their bytes as they were
    _same(got, want, "table")


@pytest.mark.parametrize("row_len,skew,wire", [(12, 0, "f32"), (72, 0, "bf16"), (64, 2, "f32"),
                                               (1544, 0, "f32")])
def test_add_is_keyed_on_the_table_row(row_len, skew, wire):
    """the same message with its rows in another order, through one block: the same table"""
    rng = np.random.default_rng([row_len, skew, len(wire)])
    keys, local, tab, src = _add_message(rng, row_len, wire, 48, 5)
    kw = dict(rounding="stochastic", seed=3, key_shift=48, row_base=5)
    first = _add(wire, tab, skew, keys, src, grid_cap=0, **kw)
    order = rng.permutation(len(keys))
    assert not np.array_equal(local[order], local)
    _same(_add(wire, tab, skew, keys[order], src[order], grid_cap=1, **kw), first, "permuted")
    _same(first, _add_model(tab, local, src, "stochastic", 3)[0], "table")


# ------------------------------------------------------------------------ (c), (d) the four steps

def _state(rng, opt, rowwise, row_len, betas):
    """Adagrad: sums in [0.01, 2]. Lazy Adam: records some steps old, p1 = beta1^j and p2 = beta2^k
    as running fp32 products with j, k in {0, 1, 7}, v_row and v in [0.01, 2], m normal"""
    if opt == "adagrad":
        return rng.uniform(0.01, 2.0, (_ROWS,) if rowwise else (_ROWS, row_len)).astype(np.float32)
    state = fresh(_ROWS, row_len, rowwise)
    for col, beta in enumerate(betas):
        steps = rng.choice([0, 1, 7], size=_ROWS)
        for i in range(7):
            state[steps > i, col] *= np.float32(beta)
    state[:, 2] = rng.uniform(0.01, 2.0, _ROWS)
    state[:, 4:4 + row_len] = rng.standard_normal((_ROWS, row_len))
    state[:, 4 + row_len:] = rng.uniform(0.01, 2.0, (_ROWS, state.shape[1] - 4 - row_len))
    return state


def _launch(kernel, tab, skew, state, keys, grad, out0, hyper, rowwise, **kw):
    """one step; (table, state, out or None) as it leaves them, inside guard bytes"""
    tab_d, st_d, grad_d, keys_d = _Dev(tab, skew), _Dev(state), _Dev(grad), _Dev(keys)
    out_d = None if out0 is None else _Dev(out0)
    getattr(ps._core, kernel)(tab_d.ptr, st_d.ptr, keys_d.ptr, len(keys), tab.shape[1], grad_d.ptr,
                              out_d.ptr if out_d else 0, *hyper, rowwise, table_rows=_ROWS, **kw)
    _same(grad_d.read(), grad, "grad")
    assert np.array_equal(keys_d.read(), keys)
    return tab_d.read(), st_d.read(), out_d.read() if out_d else None


def _both_tables(opt, rowwise, wire, skew, bits, state, keys, grad, hyper, with_out, rounding, seed,
                 **kw):
    """the step on the bf16 table and on an fp32 table holding the same weights"""
    nrows, row_len = grad.shape
    if wire == "bf16":
        kernel, g_dev, out0 = "k_sparse_%s_bf16_wire", _bits_of(grad), np.full(grad.shape, 0xABAB, np.uint16)
    else:
        kernel, g_dev, out0 = "k_sparse_%s_bf16", grad, np.full(grad.shape, np.nan, np.float32)
    got = _launch(kernel % opt, bits, skew, state, keys, g_dev, out0 if with_out else None, hyper,
                  rowwise, rounding=rounding, seed=seed, **kw)
    f32 = _launch("k_sparse_%s_f32" % opt, model.widen(bits), 0, state, keys, grad,
                  np.full(grad.shape, np.nan, np.float32) if with_out else None, hyper, rowwise, **kw)
    return got, f32


def _check_bf16(got, x, want_state, wire, bits, local, rounding, seed):
    """table bits = R(x) on the message's rows, the state's bytes, out = the stored bits (widened on
    the fp32 wire) or zeros, and everything else as it was"""
    inside, rows = local >= 0, local[local >= 0]
    tab, st, out = got
    want = bits.copy()
    want[rows] = model.store(x, _fields(rounding, seed, rows, bits.shape[1]))
    _same(tab, want, "bf16 table")
    _same(st, want_state, "state under the bf16 table")
    if out is not None:
        there = np.where(inside[:, None], want[np.maximum(local, 0)], 0).astype(np.uint16)
        _same(out, there if wire == "bf16" else model.widen(there), "out")


_STEP_LENS = [(8, 0), (24, 0), (72, 0), (1032, 0), (1544, 0), (2056, 0), (12, 0), (130, 0), (197, 0),
              (64, 2), (1032, 2)]
# (optimizer, rowwise, wire, row_len, skew, nrows, grid_cap, with_out, rounding, seed, key_shift,
# row_base): every row length with both optimizers, variants and wires; the rest take turns
_STEP_CASES = [(o, r, w, L, skew, (1, 5, 257)[i % 3], i & 1, not i & 2,
                ("stochastic", "nearest")[i % 5 == 4], _SEEDS[i % 3], 0, 0)
               for i, (o, r, w, (L, skew)) in enumerate(itertools.product(
                   ["adagrad", "lazy_adam"], [True, False], ["f32", "bf16"], _STEP_LENS))]
_STEP_CASES += [("lazy_adam", True, "f32", 72, 0, 257, 1, True, "stochastic", 3, 48, 5),
                ("adagrad", False, "bf16", 24, 0, 257, 0, True, "stochastic", 2 ** 64 - 1, 48, 5)]


@pytest.mark.parametrize("opt,rowwise,wire,row_len,skew,nrows,grid_cap,with_out,rounding,seed,shift,base",
                         _STEP_CASES)
def test_step_exact(opt, rowwise, wire, row_len, skew, nrows, grid_cap, with_out, rounding, seed, shift,
                    base):
    """Contraction-proof inputs (the module's docstring): the numpy float32 transcription of the
    operation order gives x and the new state exactly, for both files' kernels."""
    rng = np.random.default_rng([len(opt), int(rowwise), len(wire), row_len, skew, nrows, shift])
    keys, local = _keys(rng, nrows, shift, base)
    inside, rows, ins = local >= 0, local[local >= 0], np.flatnonzero(local >= 0)
    bits = model.store(rng.standard_normal((_ROWS, row_len)).astype(np.float32))
    grad = (rng.integers(-64, 65, (nrows, row_len)) / 16).astype(np.float32)
    state = _state(rng, opt, rowwise, row_len, (0.5, 0.5))
    if len(ins) > 1:  # a zero gradient (lazy Adam: on a fresh row) keeps the weight's bits
        grad[ins[0]] = 0.0
        if opt == "lazy_adam":
            state[local[ins[0]]] = fresh(1, row_len, rowwise)[0]
    hyper = (_LR, _EPS) if opt == "adagrad" else (_LR, 0.5, 0.5, _EPS)
    step = model.adagrad_step if opt == "adagrad" else model.lazy_adam_step
    x, st_rows = step(model.widen(bits[rows]), state[rows], grad[inside], *hyper, rowwise)
    want_state = state.copy()
    want_state[rows] = st_rows
    got, f32 = _both_tables(opt, rowwise, wire, skew, bits, state, keys, grad, hyper, with_out, rounding,
                            seed, key_shift=shift, row_base=base, grid_cap=grid_cap)
    # the claim of sparse_elem.h: the fp32 kernels compute the model's x and state
    want_f32 = model.widen(bits)
    want_f32[rows] = x
    _same(f32[0], want_f32, "fp32 table against the model")
    _same(f32[1], want_state, "fp32 kernel's state against the model")
    _check_bf16(got, x, want_state, wire, bits, local, rounding, seed)
    if len(ins) > 1:
        assert np.array_equal(got[0][local[ins[0]]], bits[local[ins[0]]])
    assert (_u32(x) & 0xFFFF).any() or len(ins) == 1  # the step does leave something to round


@pytest.mark.parametrize("rounding", ["stochastic", "nearest"])
@pytest.mark.parametrize("row_len", [8, 72, 130])
@pytest.mark.parametrize("opt", ["adagrad", "lazy_adam"])
def test_elementwise_step_is_the_fp32_step(opt, row_len, rounding):
    """Ordinary inputs: the element-wise bf16 kernel leaves the fp32 kernel's state bytes and R of
    the fp32 kernel's x. (Row-wise, the two files sum a row's squares in different orders.)"""
    rng = np.random.default_rng([len(opt), row_len, len(rounding)])
    keys, local = _keys(rng, 257, 0, 0)
    rows = local[local >= 0]
    bits = model.store(rng.standard_normal((_ROWS, row_len)).astype(np.float32))
    grad = rng.standard_normal((257, row_len)).astype(np.float32)
    state = _state(rng, opt, False, row_len, (_B1, _B2))
    hyper = (_LR, _EPS) if opt == "adagrad" else (_LR, _B1, _B2, _EPS)
    got, f32 = _both_tables(opt, False, "f32", 0, bits, state, keys, grad, hyper, True, rounding, 7)
    _check_bf16(got, f32[0][rows], f32[1], "f32", bits, local, rounding, 7)
