"""Torch-tensor wrappers over the MXFP8 kernels (csrc/mxfp8.hip).

The format (csrc/mxfp8.h): 512 fp32 elements pack into a 528-byte
superblock, 16 E8M0 scale bytes (one per 32 elements) followed by 512 OCP
e4m3fn codes. Synchronous, like ops.dense; the reduce-mode dense handler
with dtype="mxfp8" runs the server-side kernels on its own streams.
"""

from .. import _core


def mxfp8_packed_nbytes(n):
    """Packed bytes of n fp32 elements: ceil(n / 512) * 528."""
    return _core.mxfp8_packed_nbytes(int(n))


def _check_f32_cuda(t):
    import torch

    assert t.is_cuda, "expected a CUDA (HIP) tensor"
    assert t.dtype == torch.float32, "fp32 elements"
    assert t.is_contiguous()


def mxfp8_quantize(src, out=None):
    """Pack an fp32 tensor; returns a uint8 tensor of mxfp8_packed_nbytes(n)."""
    import torch

    _check_f32_cuda(src)
    n = src.numel()
    nbytes = mxfp8_packed_nbytes(n)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=src.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
    assert out.numel() >= nbytes
    _core.k_mx_quantize(src.data_ptr(), n, out.data_ptr())
    return out


def mxfp8_dequantize(packed, n, alpha=1.0, out=None):
    """The first n elements of a packed tensor as fp32, times alpha."""
    import torch

    assert packed.is_cuda and packed.dtype == torch.uint8 and packed.is_contiguous()
    assert packed.numel() >= mxfp8_packed_nbytes(n)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=packed.device)
    _check_f32_cuda(out)
    assert out.numel() == n
    _core.k_mx_dequantize(packed.data_ptr(), n, out.data_ptr(), float(alpha))
    return out
