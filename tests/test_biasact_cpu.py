"""relu= on Conv2dNHWC / LinearBF16 / DF.linear and DF.conv2d_bias_act on the
CPU path, and the state_dict keys of the three models that use them (the key
lists of the models before the flag: tests/golden/biasact_state_dict_keys.json)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from dtmx.models import get_symbol
from dtmx.ops import functional as DF
from dtmx.ops.layers import Conv2dNHWC, LinearBF16

GOLDEN = os.path.join(os.path.dirname(__file__), "golden",
                      "biasact_state_dict_keys.json")


@pytest.mark.parametrize("name,kw", [("vgg", {"num_layers": 16}), ("alexnet", {}),
                                     ("googlenet", {})], ids=lambda v: str(v))
def test_state_dict_keys_unchanged(name, kw):
    net = get_symbol(name, num_classes=1000, image_shape="3,224,224", **kw)
    with open(GOLDEN) as f:
        assert list(net.state_dict().keys()) == json.load(f)[name]
    assert [k for k, _ in net.named_parameters()] == list(net.state_dict().keys())


@pytest.mark.parametrize("relu", [True, False])
def test_conv_layer_equals_three_ops(relu):
    torch.manual_seed(0)
    x = torch.randn(2, 8, 9, 11, requires_grad=True)
    conv = Conv2dNHWC(8, 16, 3, 2, 1, bias=True, relu=relu)
    conv.bias.data.normal_()
    want = F.conv2d(x, conv.weight, None, 2, 1) + conv.bias.reshape(1, -1, 1, 1)
    want = F.relu(want) if relu else want
    got = conv(x)
    assert torch.equal(got, want)
    assert torch.equal(
        DF.conv2d_bias_act(x, conv.weight, conv.bias, relu, 2, 1), want)
    grads = torch.autograd.grad(got.sum(), [x, conv.weight, conv.bias])
    for a, b in zip(grads, torch.autograd.grad(want.sum(),
                                               [x, conv.weight, conv.bias])):
        assert torch.equal(a, b)


def test_linear_layer_equals_two_ops():
    torch.manual_seed(0)
    x = torch.randn(5, 24)
    fc = LinearBF16(24, 16, relu=True)
    fc.bias.data.normal_()
    want = F.relu(F.linear(x, fc.weight, fc.bias))
    assert torch.equal(fc(x), want)
    assert torch.equal(DF.linear(x, fc.weight, fc.bias, relu=True), want)
    assert torch.equal(DF.linear(x, fc.weight, fc.bias), F.linear(x, fc.weight, fc.bias))
