"""Torch model of the MXFP8 wire format (csrc/mxfp8.h), shared by
test_mxfp8_format.py and test_mxfp8_gpu.py. The model defines the format;
the host reference and the kernels are compared against it."""
import numpy as np
import torch

SUPER_ELEMS, SUPER_BYTES, BLOCK = 512, 528, 32


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
    return byte.to(torch.uint8), y.to(torch.float8_e4m3fn)


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
