"""Depthwise conv op + layer routing on the CPU (torch fallback path):
the public op matches F.conv2d(groups=C), GroupedConv2dNHWC reaches it only
for depthwise layers, and parameters / initialisation are unchanged."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from dtmx.ops import functional as DF
from dtmx.ops.layers import GroupedConv2dNHWC


def test_depthwise_conv2d_cpu_matches_torch():
    g = torch.Generator().manual_seed(0)
    for (N, C, H, W, k, stride, pad) in [(2, 16, 9, 7, 3, 1, 1), (2, 12, 8, 8, 3, 2, 0),
                                         (1, 8, 9, 9, 5, 1, 2)]:
        x = torch.randn(N, C, H, W, generator=g)
        w = torch.randn(C, 1, k, k, generator=g)
        xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        xb, wb = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        ya = DF.depthwise_conv2d(xa, wa, stride, pad)
        yb = F.conv2d(xb, wb, None, stride, pad, 1, C)
        torch.testing.assert_close(ya, yb)
        dy = torch.randn(yb.shape, generator=g)
        ya.backward(dy)
        yb.backward(dy)
        torch.testing.assert_close(xa.grad, xb.grad)
        torch.testing.assert_close(wa.grad, wb.grad)
        assert wa.grad.shape == (C, 1, k, k)


def test_depthwise_conv2d_defaults():
    x = torch.randn(1, 8, 5, 5)
    w = torch.randn(8, 1, 3, 3)
    torch.testing.assert_close(DF.depthwise_conv2d(x, w),
                               F.conv2d(x, w, None, 1, 0, 1, 8))


def _record_calls(monkeypatch):
    calls = []
    real = DF.depthwise_conv2d

    def wrapper(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(DF, "depthwise_conv2d", wrapper)
    return calls


def test_grouped_layer_routes_depthwise(monkeypatch):
    calls = _record_calls(monkeypatch)
    torch.manual_seed(0)
    layer = GroupedConv2dNHWC(32, 32, 3, 1, 1, groups=32)
    x = torch.randn(2, 32, 9, 9)
    y = layer(x)
    assert len(calls) == 1
    torch.testing.assert_close(y, F.conv2d(x, layer.weight, None, 1, 1, 1, 32))


def test_grouped_layer_non_depthwise_not_routed(monkeypatch):
    calls = _record_calls(monkeypatch)
    torch.manual_seed(0)
    layer = GroupedConv2dNHWC(32, 32, 3, 1, 1, groups=4)
    x = torch.randn(2, 32, 9, 9)
    y = layer(x)
    assert calls == []
    torch.testing.assert_close(y, F.conv2d(x, layer.weight, None, 1, 1, 1, 4))


def test_grouped_layer_depthwise_bias():
    torch.manual_seed(0)
    layer = GroupedConv2dNHWC(16, 16, 3, 2, 1, groups=16, bias=True)
    with torch.no_grad():
        layer.bias.copy_(torch.randn(16))
    x = torch.randn(2, 16, 8, 8)
    torch.testing.assert_close(
        layer(x), F.conv2d(x, layer.weight, layer.bias, 2, 1, 1, 16))


def test_state_dict_key_and_shape():
    sd = GroupedConv2dNHWC(16, 16, 3, groups=16).state_dict()
    assert list(sd.keys()) == ["weight"]
    assert tuple(sd["weight"].shape) == (16, 1, 3, 3)


def test_seeded_init_unchanged():
    torch.manual_seed(0)
    layer = GroupedConv2dNHWC(16, 16, 3, groups=16)
    torch.manual_seed(0)
    w = torch.empty(16, 1, 3, 3)
    nn.init.kaiming_normal_(w, mode="fan_in", nonlinearity="relu")
    assert torch.equal(layer.weight.detach(), w)


def test_mobilenet_cpu_forward():
    from dtmx.models import get_symbol
    torch.manual_seed(0)
    net = get_symbol("mobilenet", num_classes=10, image_shape="3,64,64").eval()
    with torch.no_grad():
        y = net(torch.randn(1, 3, 64, 64))
    assert y.shape == (1, 10)
    assert torch.isfinite(y.float()).all()
