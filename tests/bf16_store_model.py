"""Exact model of the bf16 table's store rule (the header of csrc/sparse_table.hip, "bf16 tables"
in docs/API.md) in numpy and Python ints, shared by test_bf16_store_model.py and the
test_sparse_bf16_exact*.py files. The model defines the rule; the kernels are compared with it
bit for bit.

  row_key = mix(seed + (row + 1) * phi)        row the local table row
  word(q) = mix(row_key + (q + 1) * phi)       q = e // 4, e the element's index in its row
  r       = (word >> 16 * (e % 4)) & 0xffff
  stored  = (u + r) >> 16                      u the fp32 bits; nearest: r = 0x7fff + (u >> 16 & 1)

all in 64-bit wrap-around arithmetic. Inf and NaN skip the add; a NaN whose mantissa lies in the
dropped half alone gets bit 0x40.

adagrad_step and lazy_adam_step transcribe the fp32 operation order of csrc/sparse_elem.h and of
the lazy-Adam comment in csrc/sparse_table.hip, one numpy float32 operation per stated operation.
They are exact where no product that a compiler may fuse into an add is inexact; the row's sum of
squares is taken in float64 and must be exact there too."""
import numpy as np

PHI = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1


def mix64(z):
    """the SplitMix64 finalizer on a Python int"""
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _mix64_np(z):
    """mix64 over a uint64 array (numpy's integer arrays wrap around)"""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def launch_seed(seed, n):
    """the seed of the handler's n-th rounding launch (steps and adds, from 0)"""
    return mix64(seed + (n + 1) * PHI)


def row_key(seed, row):
    return mix64(seed + (int(row) + 1) * PHI)


def r16(seed, rows, row_len):
    """(len(rows), row_len) uint32: the 16 random bits of every element of the local rows"""
    keys = np.array([row_key(seed, r) for r in rows], dtype=np.uint64)
    q = np.arange(-(-row_len // 4), dtype=np.uint64)
    words = _mix64_np(keys[:, None] + (q[None, :] + np.uint64(1)) * np.uint64(PHI))
    e = np.arange(row_len)
    fields = words[:, e // 4] >> (np.uint64(16) * (e % 4).astype(np.uint64))[None, :]
    return (fields & np.uint64(0xFFFF)).astype(np.uint32)


def store(x_f32, r16_or_none=None):
    """uint16 bits of R(x): stochastic with the given 16-bit fields, nearest-even with None"""
    u = np.ascontiguousarray(x_f32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    h, low = u >> np.uint64(16), u & np.uint64(0xFFFF)
    add = np.uint64(0x7FFF) + (h & np.uint64(1)) if r16_or_none is None \
        else np.asarray(r16_or_none).astype(np.uint64)
    rounded = (u + add) >> np.uint64(16)
    keeps_nan = ((h & np.uint64(0x7F)) == 0) & (low != 0)
    special = (u & np.uint64(0x7F800000)) == np.uint64(0x7F800000)
    return np.where(special, h | np.where(keeps_nan, np.uint64(0x40), np.uint64(0)),
                    rounded).astype(np.uint16)


def widen(bits):
    return (np.ascontiguousarray(bits).astype(np.uint32) << 16).view(np.float32)


def _f32(*xs):
    return [np.float32(x) for x in xs]


def _mean_sq(g):
    """sum(g * g) / L of every row: the sum exact in float64 (the caller's gradients make it so),
    the division one fp32 operation"""
    ss = (g.astype(np.float64) ** 2).sum(axis=1)
    assert np.array_equal(ss.astype(np.float32).astype(np.float64), ss), "sum of squares inexact"
    return ss.astype(np.float32) / np.float32(g.shape[1])


def adagrad_step(w, state, g, lr, eps, rowwise):
    """(x, state') of n rows in fp32: weights w (n, L), state (n,) row-wise or (n, L), gradients g"""
    w, state, g = (np.asarray(a, dtype=np.float32) for a in (w, state, g))
    lr, eps = _f32(lr, eps)
    s = state + (_mean_sq(g) if rowwise else g * g)
    denom = np.sqrt(s) + eps
    return w - (lr * g) / (denom[:, None] if rowwise else denom), s


def lazy_adam_step(w, rec, g, lr, beta1, beta2, eps, rowwise):
    """(x, records') of n rows in fp32; a record is {p1, p2, v_row, 0} m[L] v[L] (v element-wise
    only)"""
    w, rec, g = (np.asarray(a, dtype=np.float32) for a in (w, rec, g))
    lr, beta1, beta2, eps, one = _f32(lr, beta1, beta2, eps, 1)
    omb1, omb2 = one - beta1, one - beta2
    L, out = g.shape[1], rec.copy()
    p1, p2 = rec[:, 0] * beta1, rec[:, 1] * beta2
    alpha, c2 = (lr / (one - p1))[:, None], (one - p2)[:, None]
    m = beta1 * rec[:, 4:4 + L] + omb1 * g
    if rowwise:
        v = beta2 * rec[:, 2] + omb2 * _mean_sq(g)
        out[:, 2] = v
        v = v[:, None]
    else:
        v = beta2 * rec[:, 4 + L:] + omb2 * (g * g)
        out[:, 4 + L:] = v
    denom = np.sqrt(v / c2) + eps
    out[:, 0], out[:, 1], out[:, 4:4 + L] = p1, p2, m
    return w - (alpha * m) / denom, out
