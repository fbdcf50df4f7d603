"""Grouped conv op + layer routing on the CPU (torch fallback path): the
public op matches F.conv2d(groups=G), GroupedConv2dNHWC reaches it for
grouped, non-depthwise layers, and parameters are unchanged."""
import torch
import torch.nn.functional as F

from dtmx.ops import functional as DF
from dtmx.ops.layers import GroupedConv2dNHWC


def test_grouped_conv2d_cpu_matches_torch():
    g = torch.Generator().manual_seed(0)
    for (N, C, G, H, W, stride, pad) in [(2, 32, 8, 5, 5, 1, 1),
                                         (2, 64, 4, 7, 9, 2, 1)]:
        Cg = C // G
        x = torch.randn(N, C, H, W, generator=g)
        w = torch.randn(C, Cg, 3, 3, generator=g)
        xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        xb, wb = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        ya = DF.grouped_conv2d(xa, wa, stride, pad, G)
        yb = F.conv2d(xb, wb, None, stride, pad, 1, G)
        torch.testing.assert_close(ya, yb)
        dy = torch.randn(yb.shape, generator=g)
        ya.backward(dy)
        yb.backward(dy)
        torch.testing.assert_close(xa.grad, xb.grad)
        torch.testing.assert_close(wa.grad, wb.grad)
        assert wa.grad.shape == (C, Cg, 3, 3)


def test_grouped_conv2d_defaults():
    x = torch.randn(1, 32, 5, 5)
    w = torch.randn(32, 4, 3, 3)
    torch.testing.assert_close(DF.grouped_conv2d(x, w, groups=8),
                               F.conv2d(x, w, None, 1, 0, 1, 8))
    w1 = torch.randn(32, 32, 3, 3)
    torch.testing.assert_close(DF.grouped_conv2d(x, w1),
                               F.conv2d(x, w1, None, 1, 0, 1, 1))


def _record_calls(monkeypatch):
    calls = []
    real = DF.grouped_conv2d

    def wrapper(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(DF, "grouped_conv2d", wrapper)
    return calls


def test_grouped_layer_routes_grouped(monkeypatch):
    calls = _record_calls(monkeypatch)
    torch.manual_seed(0)
    layer = GroupedConv2dNHWC(32, 32, 3, 1, 1, groups=4)
    x = torch.randn(2, 32, 9, 9)
    y = layer(x)
    assert len(calls) == 1
    torch.testing.assert_close(y, F.conv2d(x, layer.weight, None, 1, 1, 1, 4))


def test_grouped_layer_depthwise_not_routed(monkeypatch):
    calls = _record_calls(monkeypatch)
    torch.manual_seed(0)
    layer = GroupedConv2dNHWC(32, 32, 3, 1, 1, groups=32)
    layer(torch.randn(2, 32, 9, 9))
    assert calls == []


def test_grouped_layer_bias():
    torch.manual_seed(0)
    layer = GroupedConv2dNHWC(32, 32, 3, 2, 1, groups=4, bias=True)
    with torch.no_grad():
        layer.bias.copy_(torch.randn(32))
    x = torch.randn(2, 32, 8, 8)
    torch.testing.assert_close(
        layer(x), F.conv2d(x, layer.weight, layer.bias, 2, 1, 1, 4))


def test_envelope_predicate():
    """_gconv_in_envelope is shape logic only, so it is checked here."""
    x = torch.randn(2, 64, 7, 7).bfloat16()

    def inside(C_out, Cg, k, stride, pad, groups, xx=x):
        w = torch.randn(C_out, Cg, k, k).bfloat16()
        return DF._gconv_in_envelope(xx, w, stride, pad, groups)

    assert inside(64, 16, 3, 1, 1, 4)
    assert inside(64, 4, 3, 2, 0, 16)
    assert not inside(64, 1, 3, 1, 1, 64)      # depthwise
    assert not inside(64, 64, 3, 1, 1, 1)      # dense
    assert not inside(64, 16, 5, 1, 2, 4)      # 5x5
    assert not inside(128, 16, 3, 1, 1, 4)     # C_in != C_out
    assert not inside(64, 16, 3, 3, 1, 4)      # stride 3
    assert not inside(64, 16, 3, 1, 2, 4)      # padding 2
    x48 = torch.randn(2, 48, 7, 7).bfloat16()
    assert not inside(48, 8, 3, 1, 1, 6, x48)  # C % 32 != 0
    x96 = torch.randn(2, 96, 7, 7).bfloat16()
    assert not inside(96, 12, 3, 1, 1, 8, x96)  # Cg = 12
    w = torch.randn(64, 16, 3, 3).bfloat16()
    assert DF._gconv_in_envelope(
        x, w.contiguous(memory_format=torch.channels_last), 1, 1, 4)
    assert not DF._gconv_in_envelope(x, w[:, :, :, :].transpose(2, 3), 1, 1, 4)


def test_state_dict_key_and_shape():
    sd = GroupedConv2dNHWC(64, 64, 3, groups=4).state_dict()
    assert list(sd.keys()) == ["weight"]
    assert tuple(sd["weight"].shape) == (64, 16, 3, 3)
