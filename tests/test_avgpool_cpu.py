"""Windowed average pool op + layer + model routing on the CPU (torch
fallback path): the public op is exactly F.avg_pool2d, AvgPool2dNHWC forwards
its arguments, the four Inception families reach the op with their own
count_include_pad, and their CPU results are unchanged."""
import pytest
import torch
import torch.nn.functional as F

from dtmx.ops import functional as DF
from dtmx.ops.layers import AvgPool2dNHWC


@pytest.mark.parametrize("cip", [True, False])
def test_avg_pool2d_cpu_matches_torch_bitwise(cip):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 16, 9, 7, generator=g)
    # default stride (= kernel)
    assert torch.equal(DF.avg_pool2d(x, 2, count_include_pad=cip),
                       F.avg_pool2d(x, 2, count_include_pad=cip))
    assert torch.equal(DF.avg_pool2d(x, 3, padding=1, count_include_pad=cip),
                       F.avg_pool2d(x, 3, padding=1, count_include_pad=cip))
    # explicit stride and pad, with autograd
    for (k, s, p) in [(3, 1, 1), (3, 2, 0), (5, 3, 2)]:
        xa = x.clone().requires_grad_(True)
        xb = x.clone().requires_grad_(True)
        ya = DF.avg_pool2d(xa, k, s, p, cip)
        yb = F.avg_pool2d(xb, k, s, p, False, cip)
        assert torch.equal(ya, yb)
        dy = torch.randn(yb.shape, generator=g)
        ya.backward(dy)
        yb.backward(dy)
        assert torch.equal(xa.grad, xb.grad)


def test_avg_pool2d_defaults_match_torch():
    x = torch.randn(1, 8, 6, 6)
    # count_include_pad defaults to True, as F.avg_pool2d's does
    assert torch.equal(DF.avg_pool2d(x, 3, 1, 1), F.avg_pool2d(x, 3, 1, 1))
    assert not torch.equal(DF.avg_pool2d(x, 3, 1, 1),
                           F.avg_pool2d(x, 3, 1, 1, count_include_pad=False))


def test_avg_pool2d_tuple_arguments_cpu():
    x = torch.randn(1, 8, 9, 10)
    assert torch.equal(DF.avg_pool2d(x, (3, 2), (2, 1), (1, 0), False),
                       F.avg_pool2d(x, (3, 2), (2, 1), (1, 0), False, False))


def _record_calls(monkeypatch):
    calls = []
    real = DF.avg_pool2d

    def wrapper(*a, **k):
        calls.append((a[1:], k))
        return real(*a, **k)

    monkeypatch.setattr(DF, "avg_pool2d", wrapper)
    return calls


def _norm(call):
    """(kernel, stride, padding, count_include_pad) of a recorded call."""
    a, k = call
    names = ("kernel", "stride", "padding", "count_include_pad")
    vals = dict(zip(names, (None, None, 0, True)))
    vals.update(dict(zip(names, a)))
    vals.update(k)
    return tuple(vals[n] for n in names)


def test_layer_forwards_arguments(monkeypatch):
    calls = _record_calls(monkeypatch)
    x = torch.randn(2, 8, 9, 9)
    y = AvgPool2dNHWC(3, 2, 1, count_include_pad=False)(x)
    assert [_norm(c) for c in calls] == [(3, 2, 1, False)]
    assert torch.equal(y, F.avg_pool2d(x, 3, 2, 1, False, False))
    # nn.AvgPool2d's defaults: stride = kernel, pad 0, include pad
    y = AvgPool2dNHWC(2)(x)
    assert _norm(calls[1]) == (2, None, 0, True)
    assert torch.equal(y, F.avg_pool2d(x, 2))
    assert list(AvgPool2dNHWC(3).state_dict().keys()) == []


def test_layer_exported():
    import dtmx.ops
    assert dtmx.ops.AvgPool2dNHWC is AvgPool2dNHWC


def _blocks():
    from dtmx.models import (inception_bn, inception_resnet_v2, inception_v3,
                             inception_v4)
    return [
        ("inception_bn", lambda: inception_bn.IncA(32, 8, 8, 8, 8, 8, "avg", 8),
         (1, 32, 6, 6), True),
        ("inception_v3", lambda: inception_v3.InceptionA(32, 8), (1, 32, 6, 6), False),
        ("inception_v4", lambda: inception_v4.IncA(32), (1, 32, 6, 6), False),
        ("inception_resnet_v2", lambda: inception_resnet_v2.Stem(3),
         (1, 3, 75, 75), False),
    ]


@pytest.mark.parametrize("name,make,shape,cip", _blocks(),
                         ids=[b[0] for b in _blocks()])
def test_model_pool_branch_calls_op(monkeypatch, name, make, shape, cip):
    calls = _record_calls(monkeypatch)
    torch.manual_seed(0)
    block = make().eval()
    with torch.no_grad():
        block(torch.randn(*shape))
    assert [_norm(c) for c in calls] == [(3, 1, 1, cip)]


@pytest.mark.parametrize("network,shape", [("inception-bn", (2, 3, 224, 224)),
                                           ("inception-v3", (1, 3, 299, 299))])
def test_model_cpu_forward_unchanged(monkeypatch, network, shape):
    """The model through DF.avg_pool2d equals the model with the call patched
    back to F.avg_pool2d, bit for bit, and the pool was actually reached."""
    from dtmx.models import get_symbol
    torch.manual_seed(0)
    net = get_symbol(network, num_classes=10,
                     image_shape=",".join(str(v) for v in shape[1:])).eval()
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        got = net(x)
    hits = []

    def torch_pool(x, kernel, stride=None, padding=0, count_include_pad=True):
        hits.append(1)
        return F.avg_pool2d(x, kernel, stride, padding, False, count_include_pad)

    monkeypatch.setattr(DF, "avg_pool2d", torch_pool)
    with torch.no_grad():
        want = net(x)
    assert len(hits) >= 6
    assert got.shape == (shape[0], 10) and torch.isfinite(got).all()
    assert torch.equal(got, want)


def test_envelope_rejects():
    x = torch.zeros(2, 16, 9, 9)
    env = DF._avgpool_in_envelope
    assert env(x, 3, 1, 1)
    assert env(x, 2, 2, 0) and env(x, 8, 8, 4)
    assert not env(torch.zeros(2, 20, 9, 9), 3, 1, 1)   # C % 8 != 0
    assert not env(x, 1, 1, 0)                          # K = 1
    assert not env(x, 9, 1, 0)                          # K = 9
    assert not env(x, 3, 1, 2)                          # pad > K / 2
    assert not env(x, 3, 0, 1) and not env(x, 3, 9, 1)  # stride outside 1..8
    assert not env(x, (3, 3), 1, 1)                     # tuple arguments
    assert not env(x, 3, (1, 1), 1)
    assert not env(x, 3, 1, (1, 1))
    assert not env(torch.zeros(2, 16, 2, 9), 4, 1, 0)   # empty output
    assert not env(torch.zeros(0, 16, 9, 9), 3, 1, 1)   # empty input
    assert not env(torch.zeros(16, 9, 9), 3, 1, 1)      # not 4-D


def test_fallback_key_documented():
    import dtmx.utils.env as env
    assert "avgpool" in env.__doc__
