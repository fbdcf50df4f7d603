"""The stem-conv envelope predicate and DF.conv2d's CPU path (no GPU)."""
import pytest
import torch
import torch.nn.functional as F

from dtmx.ops import functional as DF


@pytest.mark.parametrize("C,Ko,R,stride", [(3, 64, 7, 2), (8, 64, 7, 2), (3, 20, 5, 1),
                                           (3, 64, 11, 4), (3, 64, 7, 4)],
                         ids=["cpu", "C8", "Ko20", "R11", "stride4"])
def test_envelope_false_outside(C, Ko, R, stride):
    x, w = torch.randn(2, C, 32, 32), torch.randn(Ko, C, R, R)
    for t in (x, x.bfloat16()):
        assert not DF._stemconv_in_envelope(t, w.to(t.dtype), stride, R // 2, R // 2)
    assert DF._conv2d_dispatch(x, w, stride, R // 2) == "torch"


def test_conv2d_cpu_is_torch():
    x, w = torch.randn(2, 3, 9, 11), torch.randn(8, 3, 7, 7)
    assert torch.equal(DF.conv2d(x, w, 2, 3), F.conv2d(x, w, None, 2, 3))
    assert torch.equal(DF.conv2d(x, w, 2, (3, 1)), F.conv2d(x, w, None, 2, (3, 1)))
