"""Pair-valued kernel_size / padding on the CPU: DF.conv2d, Conv2dNHWC and the
factorized inception-v3 (reference symbols/inception-v3.py parameter shapes,
tests/golden/inception_v3_factorized_shapes.json)."""
import json
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from dtmx.models import inception_v3
from dtmx.ops import functional as DF
from dtmx.ops.layers import Conv2dNHWC

GOLDEN = os.path.join(os.path.dirname(__file__), "golden",
                      "inception_v3_factorized_shapes.json")
PAIRS = [((1, 7), (0, 3)), ((7, 1), (3, 0)), ((3, 3), (1, 0)), ((1, 3), (0, 0))]


@pytest.mark.parametrize("rs,pad", PAIRS, ids=lambda v: "x".join(map(str, v)))
def test_pairs_equal_torch(rs, pad):
    torch.manual_seed(0)
    x = torch.randn(2, 8, 9, 11)
    conv = Conv2dNHWC(8, 16, rs, 1, pad)
    assert tuple(conv.weight.shape) == (16, 8) + rs
    want = F.conv2d(x, conv.weight, None, 1, pad)
    assert torch.equal(conv(x), want)
    assert torch.equal(DF.conv2d(x, conv.weight, 1, pad), want)
    assert torch.equal(DF.conv2d(x, conv.weight, 1, list(pad)), want)


def test_int_module_weight_bits_unchanged():
    torch.manual_seed(7)
    conv = Conv2dNHWC(8, 16, 3, 1, 1)
    after = torch.rand(1)
    torch.manual_seed(7)
    w = torch.empty(16, 8, 3, 3)
    nn.init.kaiming_normal_(w, mode="fan_in", nonlinearity="relu")
    assert torch.equal(conv.weight, w) and torch.equal(after, torch.rand(1))
    assert conv.kernel_size == 3 and conv.padding == 1


def _conv_shapes(block):
    return [list(m.weight.shape) for m in block.modules()
            if isinstance(m, Conv2dNHWC)]


def test_factorized_blocks_have_reference_shapes():
    net = inception_v3.get_symbol(num_classes=10, factorized=True)
    with open(GOLDEN) as f:
        golden = json.load(f)
    # blocks[4] is the reference's mixed_4 (first C block), blocks[9] mixed_9
    for name, idx in (("mixed_4", 4), ("mixed_9", 9)):
        assert _conv_shapes(net.blocks[idx]) == [s for _, s in golden[name]]


def test_default_model_unchanged():
    net = inception_v3.get_symbol(num_classes=10)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert all(s[2] == s[3] for s in shapes.values() if len(s) == 4)
    assert shapes["blocks.4.b2.1.conv.weight"] == (128, 128, 3, 3)
    assert shapes["blocks.4.b3.3.conv.weight"] == (192, 128, 3, 3)
    assert shapes["blocks.9.b2b1.conv.weight"] == (384, 384, 3, 3)
    # key and parameter counts of the model before the flag existed
    assert len(shapes) == 447
    assert sum(p.numel() for p in net.parameters()) == 29085034
