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


def _check_same_len(what, a, b):
    if len(a) != len(b):
        raise ValueError(f"{what}: {len(a)} and {len(b)} entries")


def mxfp8_quantize_many(srcs, outs=None):
    """mxfp8_quantize over a list of fp32 tensors (contiguous 1-D views at
    any element offset, such as gradient buckets) in one launch per 64 of
    them; returns the list of packed uint8 tensors."""
    import torch

    srcs = list(srcs)
    if outs is not None:
        outs = list(outs)
        _check_same_len("mxfp8_quantize_many: srcs and outs", srcs, outs)
    segs = []
    result = []
    for i, src in enumerate(srcs):
        _check_f32_cuda(src)
        n = src.numel()
        nbytes = mxfp8_packed_nbytes(n)
        out = outs[i] if outs is not None else torch.empty(nbytes, dtype=torch.uint8,
                                                           device=src.device)
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
        assert out.numel() >= nbytes
        segs.append((src.data_ptr(), out.data_ptr(), n))
        result.append(out)
    _core.k_batched_mx_quantize(segs)
    return result


def mxfp8_dequantize_many(packed, ns, alpha=1.0, outs=None):
    """mxfp8_dequantize over a list of packed tensors and element counts in
    one launch per 64 of them; returns the list of fp32 tensors."""
    import torch

    packed = list(packed)
    ns = [int(n) for n in ns]
    _check_same_len("mxfp8_dequantize_many: packed and ns", packed, ns)
    if outs is not None:
        outs = list(outs)
        _check_same_len("mxfp8_dequantize_many: packed and outs", packed, outs)
    segs = []
    result = []
    for i, (p, n) in enumerate(zip(packed, ns)):
        assert p.is_cuda and p.dtype == torch.uint8 and p.is_contiguous()
        assert p.numel() >= mxfp8_packed_nbytes(n)
        out = outs[i] if outs is not None else torch.empty(n, dtype=torch.float32,
                                                           device=p.device)
        _check_f32_cuda(out)
        assert out.numel() == n
        segs.append((out.data_ptr(), p.data_ptr(), n))
        result.append(out)
    _core.k_batched_mx_dequantize(segs, float(alpha))
    return result
