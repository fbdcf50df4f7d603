"""Column-conv routing predicates and the CPU path of DF.conv2d (no GPU)."""
import pytest
import torch
import torch.nn.functional as F

import dtmx.utils.env
from dtmx.ops import functional as DF


def _ops(W=17, C=16, Ko=24, rs=(7, 1), wdtype=torch.bfloat16):
    x = torch.zeros(2, C, 17, W, dtype=torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    w = torch.zeros(Ko, C, *rs, dtype=wdtype).contiguous(
        memory_format=torch.channels_last)
    return x, w


@pytest.mark.parametrize("W", [17, 44])
def test_envelope_holds(W):
    assert DF._colconv_in_envelope(*_ops(W=W), 1, 3, 0)


@pytest.mark.parametrize("ops,stride,ph,pw", [
    (_ops(rs=(1, 7)), 1, 0, 3), (_ops(rs=(9, 1)), 1, 4, 0), (_ops(), 2, 3, 0),
    (_ops(), 1, 3, 1), (_ops(C=12), 1, 3, 0), (_ops(Ko=12), 1, 3, 0),
    (_ops(wdtype=torch.float16), 1, 3, 0), ((_ops()[0][0], _ops()[1]), 1, 3, 0),
], ids=["1x7", "T9", "stride2", "pad31", "C12", "Ko12", "dtypes", "3-D"])
def test_envelope_single_violation(ops, stride, ph, pw):
    assert not DF._colconv_in_envelope(*ops, stride, ph, pw)
    assert not DF._colconv_routed(*ops, stride, ph, pw)


def test_cpu_conv2d_unchanged():
    g = torch.Generator().manual_seed(0)
    x, w = torch.randn(2, 8, 9, 5, generator=g), torch.randn(8, 8, 7, 1, generator=g)
    assert torch.equal(DF.conv2d(x, w, 1, (3, 0)), F.conv2d(x, w, None, 1, (3, 0)))


def test_fallback_key_documented():
    assert "colconv" in dtmx.utils.env.__doc__
