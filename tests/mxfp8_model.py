"""Torch model of the MXFP8 wire format (csrc/mxfp8.h), shared by
test_mxfp8_format.py and the test_mxfp8_*gpu.py files. The model defines
the format; the host reference and the kernels are compared against it.
Below it: the format stated by hand from a table of the e4m3 values, and
the edge inputs that model, host reference and kernels are all run on."""
import numpy as np
import torch

SUPER_ELEMS, SUPER_BYTES, BLOCK = 512, 528, 32
NAN_SCALE, NAN_CODE = 0xFF, 0x7F  # a block that holds a NaN or an infinity


def packed_nbytes(n):
    return -(-n // SUPER_ELEMS) * SUPER_BYTES


def quantize(x):
    """(scale bytes uint8 [blocks], codes float8_e4m3fn [blocks, 32]) of a
    1-D fp32 CPU tensor, zero-padded to whole superblocks."""
    x = x.detach().to(torch.float32).reshape(-1)
    pad = -x.numel() % SUPER_ELEMS
    xb = torch.cat([x, torch.zeros(pad)]).view((x.numel() + pad) // BLOCK, BLOCK)
    amax = xb.abs().amax(dim=1)
    be = (amax.view(torch.int32) >> 23) & 0xff
    byte = (be - 8).clamp(min=0)
    byte = byte + (torch.ldexp(amax, 127 - byte) > 448).to(torch.int32)
    y = torch.ldexp(xb, (127 - byte)[:, None]).clamp(-448.0, 448.0)
    codes = y.to(torch.float8_e4m3fn)
    # the non-finite rule: a block with any NaN or infinity is scale byte
    # 0xFF and 32 codes 0x7F, and no other block notices
    bad = ~torch.isfinite(xb).all(dim=1)
    byte[bad] = NAN_SCALE
    codes.view(torch.uint8)[bad] = NAN_CODE
    return byte.to(torch.uint8), codes


def dequantize(byte, codes, n, alpha=None):
    v = torch.ldexp(codes.to(torch.float32), (byte.to(torch.int32) - 127)[:, None])
    v = v.reshape(-1)[:n]
    return v if alpha is None else v * torch.tensor(alpha, dtype=torch.float32)


def pack(byte, codes):
    """The model's (byte, codes) as the 528-byte-superblock byte stream."""
    nsb = byte.numel() // 16
    return torch.cat([byte.view(nsb, 16), codes.view(torch.uint8).view(nsb, SUPER_ELEMS)],
                     dim=1).reshape(-1)


def unpack(packed):
    p = torch.as_tensor(np.ascontiguousarray(packed)).view(torch.uint8)
    assert p.numel() % SUPER_BYTES == 0, p.numel()
    p = p.view(p.numel() // SUPER_BYTES, SUPER_BYTES)
    byte = p[:, :16].reshape(-1)
    codes = p[:, 16:].contiguous().view(torch.float8_e4m3fn).view(byte.numel(), BLOCK)
    return byte, codes


def roundtrip(x):
    """D(Q(x)) at x's own length."""
    byte, codes = quantize(x)
    return dequantize(byte, codes, x.numel())


def assert_packed_equal(got, want, what=""):
    """Scale bytes exactly, codes as values (so -0 == +0)."""
    gb, gc = unpack(got)
    wb, wc = unpack(want)
    assert gb.numel() == wb.numel(), (what, gb.numel(), wb.numel())
    assert torch.equal(gb, wb), (what, "scale bytes", (gb != wb).nonzero()[:4].tolist())
    n = gb.numel() * BLOCK
    assert torch.equal(dequantize(gb, gc, n), dequantize(wb, wc, n)), (what, "codes")


def same_bits_or_nan(got, want):
    """fp32 equality bit for bit, NaN equal to NaN whatever its payload."""
    got, want = got.cpu().reshape(-1), want.cpu().reshape(-1)
    gn, wn = torch.isnan(got), torch.isnan(want)
    return got.numel() == want.numel() and torch.equal(gn, wn) and torch.equal(
        got.view(torch.int32)[~gn], want.view(torch.int32)[~wn])


# ------------------------------------------------- the format stated by hand
#
# The expectation of the edge tests: numpy float64 and a table of the 127
# non-negative finite e4m3 values, no torch.float8_e4m3fn and none of
# mxfp8.h's code. The model above, the host reference and the kernels are
# all held to it byte for byte.

# codes 0x00..0x7E: multiples of 2^-9 below 2^-6, then (1 + m/8) * 2^(e-7)
E4M3_VALUES = np.array([(c & 7) * 2.0 ** -9 if c < 8 else (1 + (c & 7) / 8) * 2.0 ** ((c >> 3) - 7)
                        for c in range(127)])
assert E4M3_VALUES[1] == 2.0 ** -9 and E4M3_VALUES[126] == 448.0
assert bool((np.diff(E4M3_VALUES) > 0).all())


def hand_codes(y):
    """e4m3 code bytes of float64 values |y| <= 448: the nearest table value,
    a tie to the even code; the sign bit is the value's own, so a negative
    value that rounds to zero, -0.0 included, is 0x80."""
    y = np.asarray(y, dtype=np.float64)
    a = np.abs(y)
    assert bool((a <= 448.0).all())
    hi = np.clip(np.searchsorted(E4M3_VALUES, a), 1, 126)  # table[hi-1] <= a <= table[hi]
    lo = hi - 1
    d_lo, d_hi = a - E4M3_VALUES[lo], E4M3_VALUES[hi] - a  # exact: a has 24 bits at most
    code = np.where(d_lo < d_hi, lo, np.where(d_hi < d_lo, hi, np.where(lo % 2 == 0, lo, hi)))
    return (code | np.where(np.signbit(y), 0x80, 0)).astype(np.uint8)


def hand_decode(byte, codes):
    """fp32 values of code bytes [blocks, 32] under scale bytes [blocks],
    from the table; the NaN codes 0x7F and 0xFF give NaN."""
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1, BLOCK)
    mag = np.append(E4M3_VALUES, np.nan)[codes & 0x7F]
    v = np.where(codes & 0x80, -mag, mag) * 2.0 ** (np.asarray(byte, dtype=np.float64) - 127)[:, None]
    return torch.from_numpy(v.astype(np.float32))


def hand_quantize(x):
    """(scale bytes, code bytes [blocks, 32]) of a 1-D fp32 tensor by the
    rules of mxfp8.h's header, zero-padded to whole superblocks."""
    x = x.detach().to(torch.float32).reshape(-1).numpy()
    xb = np.concatenate([x, np.zeros(-x.size % SUPER_ELEMS, dtype=np.float32)]).reshape(-1, BLOCK)
    bad = ~np.isfinite(xb).all(axis=1)
    xd = np.where(bad[:, None], 0.0, xb).astype(np.float64)
    amax = np.abs(xd).max(axis=1)
    assert bool(((amax == 0) | ((amax >= 2.0 ** -100) & (amax <= 2.0 ** 100))).all())
    # amax = f * 2^e with f in [0.5, 1): the fp32 exponent field is e + 126
    be = np.where(amax > 0, np.frexp(amax)[1] + 126, 0)
    byte = np.maximum(be - 8, 0)
    byte = byte + (amax * 2.0 ** (127 - byte) > 448.0)
    codes = hand_codes(np.clip(xd * 2.0 ** (127 - byte)[:, None], -448.0, 448.0))
    byte[bad] = NAN_SCALE
    codes[bad] = NAN_CODE
    return torch.from_numpy(byte.astype(np.uint8)), torch.from_numpy(codes)


def hand_packed(x):
    byte, codes = hand_quantize(x)
    return pack(byte, codes)


def pad_super(x):
    """x zero-padded to whole superblocks (an accumulator's length)."""
    return torch.cat([x, torch.zeros(-x.numel() % SUPER_ELEMS)])


# ------------------------------------------------------------ edge inputs
#
# Every builder returns inputs inside the format's contract: |x| is 0 or
# lies in [2^-100, 2^100]. in_contract() is asserted by the tests.


def in_contract(x):
    a = x.abs()
    return bool(((a == 0) | ((a >= 2.0 ** -100) & (a <= 2.0 ** 100))).all())


TIE_KS = (-89, 0, 91)


def code_ties(k):
    """(x, scale bytes, code bytes [blocks, 32]) over the real blocks of x.
    Scaled by 2^-k, x holds the 127 non-negative e4m3 values, the 126
    midpoints of neighbouring values and the fp32 numbers next to each
    midpoint on either side, all with both signs, in blocks of 32 that each
    begin with 448 so that every block has the scale byte k + 127. The
    codes are stated from the construction: a value is its own code, a
    midpoint goes to the neighbour with the even code, the number above it
    to the upper code and the number below it to the lower one; a negative
    value has the sign bit, also where it rounds to zero."""
    vals, codes = [], []
    table = E4M3_VALUES.astype(np.float32)
    for c in range(127):
        vals.append(table[c])
        codes.append(c)
    for c in range(126):
        mid = np.float32((E4M3_VALUES[c] + E4M3_VALUES[c + 1]) / 2)
        assert float(mid) * 2 == E4M3_VALUES[c] + E4M3_VALUES[c + 1]
        vals += [mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(0))]
        codes += [c if c % 2 == 0 else c + 1, c + 1, c]
    vals = np.array(vals, dtype=np.float32)
    codes = np.array(codes, dtype=np.uint8)
    vals, codes = np.concatenate([vals, -vals]), np.concatenate([codes, codes | 0x80])
    pad = -vals.size % (BLOCK - 1)  # 31 values follow each block's 448
    vals = np.concatenate([vals, np.zeros(pad, dtype=np.float32)]).reshape(-1, BLOCK - 1)
    codes = np.concatenate([codes, np.zeros(pad, dtype=np.uint8)]).reshape(-1, BLOCK - 1)
    nb = vals.shape[0]
    vals = np.concatenate([np.full((nb, 1), 448.0, dtype=np.float32), vals], axis=1)
    codes = np.concatenate([np.full((nb, 1), 0x7E, dtype=np.uint8), codes], axis=1)
    x = torch.ldexp(torch.from_numpy(vals), torch.tensor(k)).reshape(-1)
    return x, torch.full((nb,), k + 127, dtype=torch.uint8), torch.from_numpy(codes)


def pack_padded(byte, codes):
    """pack() of the real blocks' bytes and codes, the padding to whole
    superblocks being zero codes under byte 0."""
    pad = -byte.numel() % 16
    return pack(torch.cat([byte, torch.zeros(pad, dtype=torch.uint8)]),
                torch.cat([codes, torch.zeros(pad, BLOCK, dtype=torch.uint8)]))


TABLE_BYTES = (0, 19, 127, 220)


def code_table(byte):
    """Two packed superblocks under one scale byte: all 256 codes, forwards
    in the first and backwards in the second, so that every code meets both
    halves of a dword and of a 16-code unit. Byte 0 heads zeros only inside
    the contract: its table is the two zero codes 0x00 and 0x80."""
    if byte == 0:
        fwd = torch.tensor([0x00, 0x80], dtype=torch.uint8).repeat(256)
    else:
        fwd = torch.arange(256, dtype=torch.int32).to(torch.uint8).repeat(2)
    codes = torch.cat([fwd, fwd.flip(0)])
    return pack(torch.full((32,), byte, dtype=torch.uint8), codes.view(32, BLOCK))


def _filler():
    """32 fixed values of magnitude 3..99, signs alternating: far enough
    below 448 that a block which lost its amax gets another scale byte."""
    i = torch.arange(BLOCK)
    return ((i * 37 % 97 + 3) * (1 - 2 * (i % 2))).to(torch.float32)


AMAX_SPOTS = (0, 15, 16, 31)
TAIL_LENS = (1, 15, 16, 17, 31)


def amax_placement(k=3):
    """Blocks alike except for where the one largest magnitude sits
    (element 0, 15, 16 or 31: either end of either lane's half), its sign
    and its scaled size, 448 (no bump) or 449 (bump)."""
    blocks = []
    for top in (448.0, 449.0):
        for sign in (1.0, -1.0):
            for spot in AMAX_SPOTS:
                b = _filler()
                b[spot] = sign * top
                blocks.append(b)
    return torch.ldexp(torch.cat(blocks), torch.tensor(k))


def amax_in_tail(rem, top, sign, k=3):
    """A superblock of filler blocks and rem more elements, the stream's
    largest-in-block magnitude at its last element n - 1."""
    x = torch.cat([_filler().repeat(16), _filler()[:rem]])
    x[-1] = sign * top
    return torch.ldexp(x, torch.tensor(k))


def contract_ends():
    """Blocks with amax exactly 2^-100 and exactly 2^100, a block of -0.0
    and a block of equal values."""
    i = torch.arange(BLOCK)
    small = torch.tensor([1.0, 0.0, -1.0, -0.0]).repeat(8) * 2.0 ** -100
    big = (i.to(torch.float32) / 32 * (1 - 2 * (i % 2))) * 2.0 ** 100
    big[5], big[22] = 2.0 ** 100, -(2.0 ** 100)
    return torch.cat([small, big, torch.full((BLOCK,), -0.0), torch.full((BLOCK,), 3.0),
                      torch.full((BLOCK,), -2.0 ** -100), torch.full((BLOCK,), 2.0 ** 100)])


def encode_cases(edge_blocks):
    """[(name, x, expected packed bytes)] of every finite edge input;
    edge_blocks is test_mxfp8_format's _edge_blocks(). The ties' codes come
    from their construction, the rest from hand_quantize()."""
    cases = []
    for k in TIE_KS:
        x, byte, codes = code_ties(k)
        cases.append((f"ties k={k}", x, pack_padded(byte, codes)))
    for name, x in (("edge blocks", edge_blocks), ("amax placement", amax_placement()),
                    ("contract ends", contract_ends())):
        cases.append((name, x, hand_packed(x)))
    for rem in TAIL_LENS:
        for top in (448.0, 449.0):
            for sign in (1.0, -1.0):
                x = amax_in_tail(rem, top, sign)
                cases.append((f"tail rem={rem} top={sign * top}", x, hand_packed(x)))
    return cases


# poisoned blocks of nonfinite_stream(): block index -> {element: value}
_NAN, _INF = float("nan"), float("inf")
POISON = {
    1: {0: _NAN}, 3: {15: _NAN}, 5: {16: _NAN}, 7: {31: _NAN},
    9: {7: _INF}, 11: {20: -_INF}, 13: {15: _NAN, 16: _INF}, 15: {0: -_INF, 31: _NAN},
    18: {3: -_NAN},
    32: {16: _NAN},  # the partial last block: its last element, n - 1
}
NONFINITE_N = 2 * SUPER_ELEMS + 17


def nonfinite_stream():
    """(finite x, poisoned x, poisoned block indices), n = 1041. The poison
    sits in every other block of the first superblock, so each poisoned
    block has finite neighbours in the lane pairs either side of it, in one
    block of the second superblock and in the 17-element last block."""
    g = torch.Generator().manual_seed(41)
    x = torch.randn(NONFINITE_N, generator=g) * torch.exp(2 * torch.randn(NONFINITE_N, generator=g))
    bad = x.clone()
    for blk, spots in POISON.items():
        for el, v in spots.items():
            bad[blk * BLOCK + el] = v
    assert torch.isnan(bad[-1]) and torch.isfinite(bad[2 * SUPER_ELEMS:-1]).all()
    return x, bad, sorted(POISON)


def poisoned_packed(finite_packed, blocks):
    """finite_packed with the given blocks replaced by the non-finite
    rule's bytes: scale 0xFF, 32 codes 0x7F."""
    byte, codes = unpack(finite_packed)
    byte, codes = byte.clone(), codes.view(torch.uint8).clone()
    byte[blocks] = NAN_SCALE
    codes[blocks] = NAN_CODE
    return pack(byte, codes)
