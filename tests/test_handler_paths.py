"""The GPU server handlers (csrc/server_handlers.cc) and the worker half
(csrc/kv_app.h) against a CPU model of the store, bit for bit.

test_kernel_shapes.py checks the kernels; this file checks the layer that
decides which kernel a message reaches: batched or per-key launches, lens
given or omitted, cmd overriding the handler's mode, entries that keep a
tail or grow, layouts taken from entry sizes, host values, skewed base
pointers, reduce rounds, the sparse table behind key_shift and device
keys, checkpoints, and an entry advert that must not outlive its entry.

Payloads come from seeded generators and differ per step, key and
element, with signed zeros, infinities, FLT_MAX pairs and exactly
cancelling pairs planted in the fp32 ones and arbitrary finite bit
patterns in the bf16 ones. They hold no NaN and never meet as inf + -inf,
so every result is compared as raw bytes. Every pull lands inside a
larger buffer of 0xAB bytes (16 before, 48 after) that is compared whole,
and every source buffer is compared after the operation.

The models and their tests at the top need no GPU; everything else is
marked gpu.

Two things stay outside the models and so outside every test: what a sum
does to an entry that grows while it holds data, and zero-length keys.
No request here is one the handlers answer with a failed check (unknown
key, destination smaller than the entries, fused push+pull on a reduce
handler). Within one sparse message the in-range rows are unique (the
handlers' contract: with one worker the scatter-add is not atomic); rows
repeat across messages, and out-of-range keys repeat within one.
"""
import struct
import threading

import numpy as np
import pytest

import ps_lite_amd as ps
from ps_lite_amd.parallel import launch_local

gpu = pytest.mark.gpu

_GUARD = 0xAB
_LEAD, _TRAIL = 16, 48  # guard bytes around every payload
_FLT_MAX = np.float32(3.4028234663852886e38)
_PORT = [30100]


# ------------------------------------------------------------------ models

def _add_bytes(a, b, dtype):
    """a + b of two equally long uint8 arrays holding fp32 or bf16."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if dtype == "f32":
        with np.errstate(over="ignore", invalid="ignore"):
            return (a.view(np.float32) + b.view(np.float32)).view(np.uint8)
    import torch

    x = torch.from_numpy(a.copy()).view(torch.bfloat16)
    y = torch.from_numpy(b.copy()).view(torch.bfloat16)
    return (x.float() + y.float()).to(torch.bfloat16).view(torch.uint8).numpy()


class StoreModel:
    """key -> bytes, following GpuDenseHandler::HandlePush / HandlePull."""

    def __init__(self, mode, dtype="f32"):
        assert mode in ("assign", "sum") and dtype in ("f32", "bf16")
        self.mode, self.dtype, self.store = mode, dtype, {}

    def sums(self, cmd):
        return cmd == 2 if self.mode == "assign" else cmd != 1

    def push(self, keys, lens_bytes, payload, cmd=0):
        payload = np.frombuffer(bytes(payload), dtype=np.uint8)
        assert int(sum(lens_bytes)) == payload.size
        off = 0
        for key, n in zip(keys, lens_bytes):
            key, n = int(key), int(n)
            assert n > 0, "zero-length keys are not modelled"
            seg = payload[off:off + n]
            cur = self.store.get(key)
            if cur is None or cur.size < n:
                assert cur is None or not self.sums(cmd), "a sum that grows an entry is not modelled"
                cur = np.zeros(n, dtype=np.uint8)  # zeroed, exactly the pushed length
            else:
                cur = cur.copy()  # at least as large: only the first n bytes change
            cur[:n] = _add_bytes(cur[:n], seg, self.dtype) if self.sums(cmd) else seg
            self.store[key] = cur
            off += n

    def pull(self, keys):
        """(concatenation of the whole entries, their sizes in bytes)"""
        ents = [self.store[int(k)] for k in keys]
        return np.concatenate(ents), [e.size for e in ents]


class SparseModel:
    """rows x row_len fp32 table: local row = (key >> key_shift) - row_base in
    wrapping uint64; rows outside the table are skipped by a scatter and
    read as zero by a gather."""

    def __init__(self, rows, row_len, accumulate, key_shift=0, row_base=0):
        self.rows, self.row_len, self.accumulate = rows, row_len, accumulate
        self.key_shift, self.row_base = key_shift, row_base
        self.table = np.zeros((rows, row_len), dtype=np.uint32)  # fp32 bit patterns

    def local_rows(self, keys):
        keys = np.asarray(keys, dtype=np.uint64)
        return (keys >> np.uint64(self.key_shift)) - np.uint64(self.row_base)

    def push(self, keys, vals, cmd=0):
        vals = np.ascontiguousarray(vals).view(np.uint32).reshape(len(keys), self.row_len)
        add = self.accumulate or cmd == 2
        for i, row in enumerate(self.local_rows(keys)):
            if row >= self.rows:
                continue
            row = int(row)
            if add:
                self.table[row] = (self.table[row].view(np.float32) +
                                   vals[i].view(np.float32)).view(np.uint32)
            else:
                self.table[row] = vals[i]

    def pull(self, keys):
        out = np.zeros((len(keys), self.row_len), dtype=np.uint32)
        for i, row in enumerate(self.local_rows(keys)):
            if row < self.rows:
                out[i] = self.table[int(row)]
        return out.reshape(-1).view(np.uint8)


def _f32(*v):
    return np.array(v, dtype=np.float32).view(np.uint8)


def test_store_model_tail_and_growth():
    m = StoreModel("assign")
    m.push([5, 9], [8, 4], _f32(1.0, 2.0, 3.0), cmd=1)
    got, sizes = m.pull([5, 9])
    assert sizes == [8, 4] and got.tobytes() == _f32(1.0, 2.0, 3.0).tobytes()
    m.push([5], [4], _f32(7.0), cmd=1)  # shorter: the tail is kept
    got, sizes = m.pull([5])
    assert sizes == [8] and got.tobytes() == _f32(7.0, 2.0).tobytes()
    m.push([5], [12], _f32(4.0, 5.0, 6.0), cmd=1)  # longer: zeroed and replaced
    got, sizes = m.pull([9, 5])
    assert sizes == [4, 12] and got.tobytes() == _f32(3.0, 4.0, 5.0, 6.0).tobytes()
    with pytest.raises(AssertionError):
        m.push([9], [8], _f32(1.0, 1.0), cmd=2)  # a sum that grows: not modelled


def test_store_model_cmd_overrides_mode():
    a = StoreModel("assign")
    a.push([1], [8], _f32(1.5, -0.0), cmd=0)
    a.push([1], [8], _f32(2.0, -0.0), cmd=0)  # assign handler: default assigns
    assert a.pull([1])[0].tobytes() == _f32(2.0, -0.0).tobytes()
    a.push([1], [8], _f32(0.25, 0.0), cmd=2)  # cmd=2 sums on it; -0 + +0 = +0
    assert a.pull([1])[0].tobytes() == _f32(2.25, 0.0).tobytes()
    s = StoreModel("sum")
    s.push([1], [8], _f32(1.5, -0.0), cmd=0)  # first push: zeros + payload, so -0 turns +0
    assert s.pull([1])[0].tobytes() == _f32(1.5, 0.0).tobytes()
    s.push([1], [8], _f32(1.5, float("inf")), cmd=2)
    assert s.pull([1])[0].tobytes() == _f32(3.0, float("inf")).tobytes()
    s.push([1], [4], _f32(-8.0), cmd=1)  # cmd=1 assigns on a sum handler, tail kept
    assert s.pull([1])[0].tobytes() == _f32(-8.0, float("inf")).tobytes()
    big = float(_FLT_MAX)
    s.push([2], [8], _f32(big, 3.0), cmd=0)
    s.push([2], [8], _f32(big, -3.0), cmd=0)  # overflow to inf, exact cancellation to +0
    assert s.pull([2])[0].tobytes() == _f32(float("inf"), 0.0).tobytes()


def test_store_model_bf16_rounds_to_nearest_even():
    m = StoreModel("sum", "bf16")
    one, one_ulp, half_ulp = 0x3F80, 0x3F81, 0x3B80  # 1, 1 + 2^-7, 2^-8
    m.push([3], [4], np.array([one, one_ulp], dtype=np.uint16).view(np.uint8))
    m.push([3], [4], np.array([half_ulp, half_ulp], dtype=np.uint16).view(np.uint8))
    got = m.pull([3])[0].view(np.uint16).tolist()
    assert got == [0x3F80, 0x3F82]  # both ties: down to even 1.0, up to even 1 + 2^-6


def test_sparse_model_by_hand():
    m = SparseModel(rows=4, row_len=2, accumulate=False)
    top = 2 ** 64 - 1
    m.push([1, 4, top, 3], np.arange(8, dtype=np.float32), cmd=0)  # rows 4 and 2^64-1 skipped
    got = m.pull([3, 1, 4, 0, top]).view(np.float32).tolist()
    assert got == [6.0, 7.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    m.push([3], np.array([1.0, -7.0], dtype=np.float32), cmd=2)  # cmd=2 adds
    m.push([3], np.array([5.0, 5.0], dtype=np.float32), cmd=0)  # cmd=0 assigns here
    assert m.pull([3]).view(np.float32).tolist() == [5.0, 5.0]
    acc = SparseModel(rows=4, row_len=2, accumulate=True, key_shift=4, row_base=2)
    keys = [(2 << 4) | 9, (5 << 4) | 1, (6 << 4), (1 << 4)]  # local rows 0, 3, 4 and a wrapped one
    for _ in range(2):
        acc.push(keys, np.arange(8, dtype=np.float32), cmd=0)  # accumulates whatever the cmd
    assert acc.pull(keys).view(np.float32).tolist() == [0.0, 2.0, 4.0, 6.0, 0.0, 0.0, 0.0, 0.0]


# ---------------------------------------------------------------- payloads

def payload_f32(seed, step, n):
    """n fp32 values as bytes. Every third element holds an edge value
    whose kind and sign depend on the position alone, so that summing
    payloads of any steps never adds inf to -inf; the cancelling kind
    changes sign with the step's parity."""
    x = np.random.default_rng([seed, step]).standard_normal(n).astype(np.float32)
    fixed = np.random.default_rng([seed, 77]).standard_normal(n).astype(np.float32)
    at = np.arange(1, n, 3)
    kind = (at // 3) % 9
    inf = np.float32(np.inf)
    even = step % 2 == 0
    for k, v in ((0, np.float32(0.0)), (1, np.float32(-0.0)), (2, inf), (3, -inf),
                 (4, _FLT_MAX), (5, -_FLT_MAX)):
        x[at[kind == k]] = v
    sel = at[kind == 6]
    x[sel] = fixed[sel] if even else -fixed[sel]
    if even:
        x[at[kind == 7]] = inf  # inf meets a finite value of the odd steps
    x[at[kind == 8]] = np.float32(-0.0) if even else np.float32(0.0)
    assert not np.isnan(x).any()
    return x.view(np.uint8)


def payload_bf16(seed, step, n):
    """n bf16 values as bytes: any finite bit pattern."""
    bits = np.random.default_rng([seed, step, 16]).integers(0, 1 << 16, n, dtype=np.uint32)
    bits = bits.astype(np.uint16)
    bits[(bits & 0x7F80) == 0x7F80] ^= 0x0080  # exponent all ones: inf or NaN
    return bits.view(np.uint8)


def _payload(dtype, seed, step, units):
    """`units` 4-byte units of payload."""
    return payload_f32(seed, step, units) if dtype == "f32" else payload_bf16(seed, step, 2 * units)


def _u64(keys):
    return np.array([int(k) for k in keys], dtype=np.uint64)


def _i32(lens):
    return np.array(lens, dtype=np.int32)


class _Buf:
    """A pool (or host pool) buffer: 16 + skew guard bytes, the payload
    range, 48 guard bytes. ptr names the payload range."""

    def __init__(self, mod, payload, skew=0, host=False):
        if isinstance(payload, (int, np.integer)):
            payload = np.full(int(payload), _GUARD, dtype=np.uint8)
        self.lead, self.n = _LEAD + skew, payload.size
        self.image = np.full(self.lead + self.n + _TRAIL, _GUARD, dtype=np.uint8)
        self.image[self.lead:self.lead + self.n] = payload
        assert self.image.size % 4 == 0
        self.buf = (mod.host_alloc if host else mod.pool_alloc)(self.image.size)
        assert host or self.buf.ptr % 16 == 0
        self.buf.copy_from(self.image)
        self.ptr, self.device = self.buf.ptr + self.lead, -1 if host else 0

    def read(self):
        return self.buf.to_numpy_f32().view(np.uint8)[:self.image.size].copy()

    def check_unchanged(self, what):
        assert np.array_equal(self.read(), self.image), "%s: source buffer changed" % what

    def check_holds(self, payload, what):
        expect = self.image.copy()
        expect[self.lead:self.lead + self.n] = payload
        got = self.read()
        if not np.array_equal(got, expect):
            bad = np.flatnonzero(got != expect)
            at = int(bad[0])
            raise AssertionError(
                "%s: %d bytes differ, first at byte %d (payload %d..%d): got %s want %s"
                % (what, bad.size, at, self.lead, self.lead + self.n,
                   got[max(0, at - 4):at + 12].tolist(), expect[max(0, at - 4):at + 12].tolist()))


# ------------------------------------------------- in-process joint node

class _Node:
    """One scheduler plus one joint worker+server in this process, a GPU
    dense handler and its model in step."""

    def __init__(self, mode, dtype="f32"):
        self.mode, self.dtype = mode, dtype

    def __enter__(self):
        _PORT[0] += 7
        ps.setup_env(1, 1, root_port=_PORT[0], XPS_DEV_ID=0, XPS_POOL_GB=4)
        ths = [threading.Thread(target=ps.start, kwargs=dict(role="scheduler", device=-1)),
               threading.Thread(target=ps.start, kwargs=dict(role="joint", device=0))]
        [t.start() for t in ths]
        [t.join() for t in ths]
        self.server = ps.KVServer(0)
        if self.mode != "sparse":
            self.server.set_gpu_dense_handle(mode=self.mode, dtype=self.dtype)
            self.model = StoreModel(self.mode, self.dtype)
        self.worker = ps.KVWorker(0, 0)
        return self

    def __exit__(self, *exc):
        ths = [threading.Thread(target=ps.finalize, kwargs=dict(role="scheduler")),
               threading.Thread(target=ps.finalize, kwargs=dict(role="joint"))]
        [t.start() for t in ths]
        [t.join() for t in ths]
        ps.clear_registry()
        return False

    def push(self, keys, lens, payload, cmd, with_lens=True, skew=0, host=False, what=""):
        """lens in 4-byte units, as on the wire."""
        src = _Buf(ps, payload, skew, host)
        w = self.worker
        w.wait(w.zpush_ptr(_u64(keys), src.ptr, src.n, src.device,
                           _i32(lens if with_lens else []), cmd=cmd))
        src.check_unchanged(what)
        self.model.push(keys, [4 * n for n in lens], payload, cmd)

    def pull(self, keys, lens, with_lens=True, skew=0, host=False, what=""):
        """Pull into a destination sized and lens-ed for `lens`; the model
        says what must arrive."""
        expect, sizes = self.model.pull(keys)
        assert sizes == [4 * n for n in lens], "the test sized its destination wrongly"
        dst = _Buf(ps, expect.size, skew, host)
        w = self.worker
        w.wait(w.zpull_ptr(_u64(keys), dst.ptr, dst.n, dst.device,
                           _i32(lens if with_lens else [])))
        dst.check_holds(expect, what)

    def pushpull(self, keys, lens, payload, cmd, what=""):
        src, dst = _Buf(ps, payload), _Buf(ps, payload.size)
        w = self.worker
        w.wait(w.zpushpull_ptr(_u64(keys), src.ptr, dst.ptr, src.n, 0, _i32(lens), cmd=cmd))
        src.check_unchanged(what)
        self.model.push(keys, [4 * n for n in lens], payload, cmd)
        dst.check_holds(self.model.pull(keys)[0], what)


# floats (4-byte units) per key, and whether the messages carry lens
_LAYOUTS = {
    "batched": ([4, 1028, 260, 2052], True),       # batched launch, unequal lengths
    "per_key": ([1028, 3, 260], True),             # per-key loop, later sources skewed
    "no_lens_1028": ([1028] * 3, False),           # equal split, batched
    "no_lens_1027": ([1027] * 3, False),           # equal split, per-key
    "keys_130": ([(4, 8, 12, 516)[i % 4] for i in range(130)], True),  # three launches
    "one_1": ([1], True),
    "one_3": ([3], True),
    "one_4": ([4], True),
    "one_4099": ([4099], True),
}
_MULTI = ["batched", "per_key", "no_lens_1028", "no_lens_1027", "keys_130"]
_SINGLE = ["one_1", "one_3", "one_4", "one_4099"]


def _keys_of(name, lens):
    base = 1000 * (1 + list(_LAYOUTS).index(name))
    return [base + 3 * i for i in range(len(lens))]


def _sequence(node, name, seq, seed, **kw):
    """One of the push/pull sequences of a layout on a node. seq is a list
    of (cmd, number of pushes before the pull)."""
    lens, with_lens = _LAYOUTS[name]
    keys = _keys_of(name, lens)
    step = 0
    for cmd, pushes in seq:
        for _ in range(pushes):
            what = "%s %s step %d cmd %d" % (node.mode, name, step, cmd)
            node.push(keys, lens, _payload(node.dtype, seed, step, sum(lens)), cmd,
                      with_lens=with_lens, what=what, **kw)
            step += 1
        node.pull(keys, lens, with_lens=with_lens, what=what + " pull", **kw)
    return keys, lens


_ASSIGN_SEQ = [(1, 1), (2, 1), (1, 1)]  # assign, pull; sum on the same keys, pull; assign, pull
_SUM_SEQ = [(0, 3), (1, 1)]             # three default pushes, pull; assign, pull


@gpu
@pytest.mark.parametrize("name", _MULTI + _SINGLE)
def test_dense_assign_handler(name):
    with _Node("assign") as node:
        _sequence(node, name, _ASSIGN_SEQ, seed=11)


@gpu
@pytest.mark.parametrize("name", _MULTI + _SINGLE)
def test_dense_sum_handler(name):
    with _Node("sum") as node:
        _sequence(node, name, _SUM_SEQ, seed=12)


@gpu
@pytest.mark.parametrize("name", _MULTI[:3] + _SINGLE)
def test_dense_sum_handler_bf16(name):
    with _Node("sum", "bf16") as node:
        _sequence(node, name, _SUM_SEQ, seed=13)


@gpu
@pytest.mark.parametrize("name", ["batched", "per_key"])
def test_dense_fused_rounds(name):
    """Fused push+pull on the sum handler: every round returns the running sum."""
    lens, _ = _LAYOUTS[name]
    keys = _keys_of(name, lens)
    with _Node("sum") as node:
        for step in range(3):
            node.pushpull(keys, lens, payload_f32(14, step, sum(lens)), cmd=0,
                          what="fused %s round %d" % (name, step))


@gpu
def test_dense_shorter_then_longer():
    """A shorter push keeps the entry's tail, a longer one replaces it, and
    a multi-key pull lays its segments out by the entry sizes."""
    a, b = 501, 502
    with _Node("assign") as node:
        node.push([a, b], [260, 1028], payload_f32(15, 0, 1288), cmd=1, what="first")
        node.push([a], [100], payload_f32(15, 1, 100), cmd=1, what="shorter")
        node.pull([a], [260], what="whole entry after the shorter push")
        node.push([a], [516], payload_f32(15, 2, 516), cmd=1, what="longer")
        node.pull([a, b], [516, 1028], what="layout from entry sizes")
        node.pull([b, a], [1028, 516], what="layout from entry sizes, reversed")


@gpu
@pytest.mark.parametrize("mode,seq", [("assign", _ASSIGN_SEQ), ("sum", _SUM_SEQ)])
def test_dense_host_values(mode, seq):
    """Values pushed from and pulled into host-pool buffers."""
    with _Node(mode) as node:
        for name in ("per_key", "one_4099"):
            keys, lens = _sequence(node, name, seq, seed=16, host=True)
            node.pull(keys, lens, what="%s %s device pull of host pushes" % (mode, name))


@gpu
@pytest.mark.parametrize("mode,seq", [("assign", _ASSIGN_SEQ), ("sum", _SUM_SEQ)])
def test_dense_skewed_base(mode, seq):
    """Worker buffers 4 bytes off a 16-byte boundary: every length and
    running offset is a 16-byte multiple, the pointers are not, so the
    handlers must take the per-key launchers."""
    with _Node(mode) as node:
        _sequence(node, "batched", seq, seed=17, skew=4)


def _read_dense_checkpoint(path):
    raw = open(path, "rb").read()
    (n,), at, out = struct.unpack_from("<Q", raw, 0), 8, {}
    for _ in range(n):
        key, size = struct.unpack_from("<QQ", raw, at)
        out[key] = np.frombuffer(raw, dtype=np.uint8, count=size, offset=at + 16).copy()
        at += 16 + size
    assert at == len(raw), "trailing bytes in the checkpoint"
    return out


@gpu
def test_dense_checkpoint(tmp_path):
    path = str(tmp_path / "dense.ckpt")
    with _Node("assign") as node:
        sets = [_sequence(node, name, _ASSIGN_SEQ, seed=18) for name in ("per_key", "one_4099")]
        node.server.save_checkpoint(path)
        saved = _read_dense_checkpoint(path)
        assert sorted(saved) == sorted(node.model.store)
        for key, want in node.model.store.items():
            assert saved[key].size == want.size and np.array_equal(saved[key], want), key
        for keys, lens in sets:  # overwrite every key, then restore
            node.push(keys, lens, payload_f32(19, 0, sum(lens)), cmd=1, what="overwrite")
            node.pull(keys, lens, what="overwritten")
        node.server.load_checkpoint(path)
        node.model.store = {k: v.copy() for k, v in saved.items()}
        for keys, lens in sets:
            node.pull(keys, lens, what="restored from the checkpoint")


# ------------------------------------------------------------------ sparse

_ROWS = 64


def _sparse_keys(rng, nkeys, unique_rows):
    """nkeys keys in random order: in-range rows (unique within the
    message) mixed with keys at `rows`, above it, and 2^64 - 1."""
    if nkeys == 1:
        return _u64([int(rng.integers(0, _ROWS))])
    n_in = int(rng.integers(_ROWS // 2, _ROWS + 1))
    inside = rng.choice(_ROWS, size=n_in, replace=False)
    beyond = [_ROWS, _ROWS + 1, _ROWS + 12345, 2 ** 63, 2 ** 64 - 1]
    outside = [beyond[i] for i in rng.integers(0, len(beyond), nkeys - n_in)]
    keys = [int(k) for k in inside] + outside
    rng.shuffle(keys)
    return _u64(keys)


def _sparse_vals(rng, case, n):
    if case == "assign":  # any bit pattern at all
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.uint8)
    return rng.integers(-1024, 1025, n).astype(np.float32).view(np.uint8)  # exact in any order


def _read_sparse_checkpoint(path, rows, row_len):
    raw = open(path, "rb").read()
    hdr = struct.unpack_from("<QQQ", raw, 0)
    assert hdr[:2] == (rows, row_len) and len(raw) == 24 + rows * row_len * 4
    return np.frombuffer(raw, dtype=np.uint32, offset=24).reshape(rows, row_len)


@gpu
@pytest.mark.parametrize("case", ["assign", "add", "accumulate"])
@pytest.mark.parametrize("nkeys", [1, 257])
@pytest.mark.parametrize("row_len", [3, 8])
def test_sparse_handler(row_len, nkeys, case, tmp_path):
    """assign: cmd=0 on a non-accumulating table; add: cmd=2 on it;
    accumulate: cmd=0 on an accumulating one. Each with host and device
    keys, as push-then-pull and as one fused push+pull; then a checkpoint."""
    cmd = 2 if case == "add" else 0
    rng = np.random.default_rng([row_len, nkeys, len(case)])
    with _Node("sparse") as node:
        node.server.set_gpu_sparse_handle(_ROWS, row_len, accumulate=(case == "accumulate"))
        model = SparseModel(_ROWS, row_len, accumulate=(case == "accumulate"))
        w = node.worker

        def round_(keys, vals, dev_keys, fused, what):
            lens = _i32([row_len] * len(keys))
            kbuf = _Buf(ps, keys.view(np.uint8)) if dev_keys else None
            kptr = kbuf.ptr if dev_keys else 0
            src, dst = _Buf(ps, vals), _Buf(ps, vals.size)
            if fused:
                w.wait(w.zpushpull_ptr(keys, src.ptr, dst.ptr, src.n, 0, lens, cmd=cmd,
                                       keys_dev_ptr=kptr))
            else:
                w.wait(w.zpush_ptr(keys, src.ptr, src.n, 0, lens, cmd=cmd, keys_dev_ptr=kptr))
                w.wait(w.zpull_ptr(keys, dst.ptr, dst.n, 0, lens, keys_dev_ptr=kptr))
            model.push(keys, vals, cmd)
            dst.check_holds(model.pull(keys), what)
            src.check_unchanged(what)
            if kbuf:
                kbuf.check_unchanged(what + " (keys)")

        def gather(keys, what):
            dst = _Buf(ps, len(keys) * row_len * 4)
            w.wait(w.zpull_ptr(keys, dst.ptr, dst.n, 0, _i32([row_len] * len(keys))))
            dst.check_holds(model.pull(keys), what)

        for dev_keys in (False, True):
            for fused in (False, True):
                keys = _sparse_keys(rng, nkeys, True)
                what = "%s row_len=%d nkeys=%d dev_keys=%s fused=%s" % (case, row_len, nkeys,
                                                                       dev_keys, fused)
                round_(keys, _sparse_vals(rng, case, nkeys * row_len), dev_keys, fused, what)
        every = _u64(list(range(_ROWS)) + [_ROWS, 2 ** 64 - 1])
        gather(every, "whole table")
        if nkeys == 1:
            gather(_u64([_ROWS]), "single key just past the table")
        # checkpoint: save, scatter more, load, gather the saved state back
        path = str(tmp_path / "sparse.ckpt")
        node.server.save_checkpoint(path)
        assert np.array_equal(_read_sparse_checkpoint(path, _ROWS, row_len), model.table)
        saved = model.table.copy()
        keys = _sparse_keys(rng, nkeys, True)
        round_(keys, _sparse_vals(rng, case, nkeys * row_len), False, False, "after the save")
        node.server.load_checkpoint(path)
        model.table = saved
        gather(every, "restored from the checkpoint")


# ------------------------------------------------- two joint processes

_HALF = 1 << 63


def _reduce_rounds(ps_mod, rank, dtype, lens, seed):
    """Three overlapped push+pull rounds of one multi-key message; each
    rank derives both payloads and expects their sum (the add commutes, so
    the arrival order does not matter)."""
    server = ps_mod.KVServer(0)
    server.set_gpu_dense_handle(mode="reduce", dtype=dtype)
    ps_mod.barrier("worker", ps_mod.WORKER_GROUP)
    worker = ps_mod.KVWorker(0, 0)
    keys = _u64([41 + i for i in range(len(lens))])
    for rnd in range(3):
        mine, theirs = (_payload(dtype, seed, 2 * rnd + r, sum(lens)) for r in (rank, 1 - rank))
        src, dst = _Buf(ps_mod, mine), _Buf(ps_mod, mine.size)
        ts1 = worker.zpush_ptr(keys, src.ptr, src.n, 0, _i32(lens))
        ts2 = worker.zpull_ptr(keys, dst.ptr, dst.n, 0, _i32(lens))  # overlapped, no barrier
        worker.wait(ts1)
        worker.wait(ts2)
        dst.check_holds(_add_bytes(mine, theirs, dtype), "reduce %s round %d rank %d"
                        % (dtype, rnd, rank))
        src.check_unchanged("reduce round %d" % rnd)
    return "ok", server


def _reduce_f32_fn(ps_mod, rank):
    # the 3-float bucket is no 16-byte multiple: per-key launches on the
    # push, the staging branch on the pull
    return _reduce_rounds(ps_mod, rank, "f32", [1024, 3, 4096, 64], seed=21)


def _reduce_one_3_fn(ps_mod, rank):
    # a group of one key, 12 bytes: the staging pull answers with a view of the entry
    return _reduce_rounds(ps_mod, rank, "f32", [3], seed=25)


def _reduce_one_1024_fn(ps_mod, rank):
    # a group of one key, 16-byte multiple: the in-place batched pull of one segment
    return _reduce_rounds(ps_mod, rank, "f32", [1024], seed=26)


def _reduce_bf16_fn(ps_mod, rank):
    return _reduce_rounds(ps_mod, rank, "bf16", [1024, 64, 2048], seed=22)


def _two_procs(fn):
    results = launch_local(2, 2, fn, joint=True, devices={0: 0, 1: 0},
                           env_extra={"XPS_POOL_GB": 4}, timeout=300)
    assert results == {0: "ok", 1: "ok"}, results


@gpu
def test_reduce_rounds_f32_two_procs():
    for fn in (_reduce_f32_fn, _reduce_one_3_fn, _reduce_one_1024_fn):
        _two_procs(fn)


@gpu
def test_reduce_rounds_bf16_two_procs():
    _two_procs(_reduce_bf16_fn)


def _sparse_shift_fn(ps_mod, rank):
    """key = row << 48 over two servers of 64 rows: server 1 has a
    non-zero row_base. Each rank owns the local rows of its parity on both
    servers; one key per server names local row 64 and must read zero."""
    shift = 48
    server = ps_mod.KVServer(0)
    worker = None
    for row_len in (5, 8):
        server.set_gpu_sparse_handle(_ROWS, row_len, accumulate=False, key_shift=shift)
        ps_mod.barrier("worker", ps_mod.WORKER_GROUP)  # both tables are up
        worker = worker or ps_mod.KVWorker(0, 0)
        rng = np.random.default_rng([23, row_len, rank])
        bases = [0, _HALF >> shift]
        rows = [b + r for b in bases for r in list(range(rank, _ROWS, 2)) + [_ROWS]]
        junk = rng.integers(0, 1 << shift, len(rows), dtype=np.uint64)
        keys = _u64([(r << shift) | int(j) for r, j in zip(rows, junk)])  # sorted: rows ascend
        assert np.all(keys[1:] > keys[:-1])
        vals = rng.integers(0, 1 << 32, len(keys) * row_len,
                            dtype=np.uint64).astype(np.uint32).view(np.uint8)
        expect = vals.copy().reshape(len(keys), row_len * 4)
        for i, r in enumerate(rows):
            if r - bases[r >= bases[1]] >= _ROWS:
                expect[i] = 0
        lens = _i32([row_len] * len(keys))
        src, dst = _Buf(ps_mod, vals), _Buf(ps_mod, vals.size)
        worker.wait(worker.zpush_ptr(keys, src.ptr, src.n, 0, lens, cmd=0))
        worker.wait(worker.zpull_ptr(keys, dst.ptr, dst.n, 0, lens))
        dst.check_holds(expect.reshape(-1), "key_shift row_len=%d rank %d" % (row_len, rank))
        src.check_unchanged("key_shift push")
        ps_mod.barrier("worker", ps_mod.WORKER_GROUP)  # nobody still uses this table
    return "ok", server


@gpu
def test_sparse_key_shift_two_servers():
    _two_procs(_sparse_shift_fn)


def _stale_advert_fn(ps_mod, rank):
    """A multi-key push grows key a after the worker cached a's entry
    advert from a single-key push. The next single-key push of the old
    length must still reach the store."""
    server = ps_mod.KVServer(0)
    server.set_gpu_dense_handle(mode="assign")
    ps_mod.barrier("worker", ps_mod.WORKER_GROUP)
    worker = ps_mod.KVWorker(0, 0)
    n = 1028
    base = (1 - rank) * _HALF  # the other rank's server
    a, b = base + 10, base + 20
    p = [payload_f32(24, step, units) for step, units in enumerate((n, n, 3 * n, n))]
    srcs = [_Buf(ps_mod, x) for x in p]
    dst1, dst2 = _Buf(ps_mod, 4 * n), _Buf(ps_mod, 8 * n)  # nothing is allocated below
    ka, kab = _u64([a]), _u64([a, b])
    for i in (0, 1):  # the second push finds the advert and goes one-sided
        worker.wait(worker.zpush_ptr(ka, srcs[i].ptr, 4 * n, 0, _i32([n]), cmd=1))
    worker.wait(worker.zpull_ptr(ka, dst1.ptr, 4 * n, 0, _i32([n])))
    dst1.check_holds(p[1], "pull after the one-sided push")
    worker.wait(worker.zpush_ptr(kab, srcs[2].ptr, 12 * n, 0, _i32([2 * n, n]), cmd=1))
    worker.wait(worker.zpush_ptr(ka, srcs[3].ptr, 4 * n, 0, _i32([n]), cmd=1))
    worker.wait(worker.zpull_ptr(ka, dst2.ptr, 8 * n, 0, _i32([2 * n])))
    dst2.check_holds(np.concatenate([p[3], p[2][4 * n:8 * n]]),
                     "single-key push after a multi-key growth, rank %d" % rank)
    for s in srcs:
        s.check_unchanged("stale advert")
    return "ok", server


@gpu
def test_advert_does_not_outlive_entry_two_procs():
    _two_procs(_stale_advert_fn)
