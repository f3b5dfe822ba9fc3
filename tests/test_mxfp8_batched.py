"""The batched worker-side MXFP8 pair, as far as it goes without a GPU:
empty lists launch nothing, the ops wrappers check their arguments before
any kernel, and PSGradSync takes mx_batched."""
import pytest
import torch

import ps_lite_amd as ps
from ps_lite_amd import ops
from ps_lite_amd.parallel.dp import PSGradSync

_core = ps._core


def test_empty_lists_launch_nothing():
    assert _core.k_batched_mx_quantize([]) == 0
    assert _core.k_batched_mx_dequantize([]) == 0
    assert _core.k_batched_mx_quantize([], tile_cap=3) == 0
    assert _core.k_batched_mx_dequantize([], alpha=0.5, tile_cap=1) == 0
    # empty segments only: nothing to launch either, whatever the pointers
    assert _core.k_batched_mx_quantize([(0, 0, 0), (4, 16, 0)]) == 0
    assert _core.k_batched_mx_dequantize([(0, 0, 0), (4, 16, 0)]) == 0
    assert ops.mxfp8_quantize_many([]) == []
    assert ops.mxfp8_dequantize_many([], []) == []


def test_bad_arguments_raise_before_any_launch():
    # checked over the whole list first, so no GPU is needed to see them
    with pytest.raises(ValueError):
        _core.k_batched_mx_quantize([(0, 0, 0), (16, 8, 4)])
    with pytest.raises(ValueError):
        _core.k_batched_mx_dequantize([(0, 0, 0), (0, 16, 4)])


def test_many_wrappers_check_list_lengths_first():
    x = torch.zeros(8)  # a CPU tensor: the length check comes before it is looked at
    p = torch.zeros(528, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.mxfp8_quantize_many([x, x], outs=[p])
    with pytest.raises(ValueError):
        ops.mxfp8_dequantize_many([p], [8, 8])
    with pytest.raises(ValueError):
        ops.mxfp8_dequantize_many([p, p], [8, 8], outs=[x])


def test_many_wrappers_reject_cpu_tensors():
    x = torch.zeros(8)
    p = torch.zeros(528, dtype=torch.uint8)
    with pytest.raises(AssertionError):
        ops.mxfp8_quantize_many([x])
    with pytest.raises(AssertionError):
        ops.mxfp8_dequantize_many([p], [8])


def test_gradsync_takes_mx_batched_without_compress():
    params = [torch.nn.Parameter(torch.zeros(10))]
    for flag in (False, True):
        sync = PSGradSync(ps, None, params, num_workers=1, mx_batched=flag)
        assert sync.compress is None and sync.mx_batched is flag
        assert sync.mx_launches == 0
