"""want_stats on the torch path (CPU, fp32): the torch result and two empty
slabs; GroupedConv2dNHWC attaches nothing there."""
import pytest
import torch
import torch.nn.functional as F

from dtmx.ops import functional as DF
from dtmx.ops.layers import GroupedConv2dNHWC


@pytest.mark.parametrize("groups", [32, 4], ids=["depthwise", "grouped"])
def test_want_stats_cpu(groups):
    torch.manual_seed(0)
    x = torch.randn(2, 32, 7, 9)
    w = torch.randn(32, 32 // groups, 3, 3)
    if groups == 32:
        y, ps, pss = DF.depthwise_conv2d(x, w, 2, 1, want_stats=True)
    else:
        y, ps, pss = DF.grouped_conv2d(x, w, 2, 1, groups, want_stats=True)
    torch.testing.assert_close(y, F.conv2d(x, w, None, 2, 1, 1, groups))
    assert ps.numel() == 0 and pss.numel() == 0
    layer = GroupedConv2dNHWC(32, 32, 3, 2, 1, groups=groups).train()
    assert not hasattr(layer(x), "_dtmx_bn_stats")
