"""Wrapper-level logic of the elementwise ops that needs no GPU.

relu_fwd / relu_bwd / add_relu_fwd walk their operands' storage linearly, so
the Python side must hand them dense tensors that share one layout. These
tests pin the layout helpers of dtmx/ops/functional.py on the stride patterns
autograd really produces: torch.cat's backward hands each branch a channel
narrow of the upstream gradient, reshape's backward an NCHW block.
"""
import pytest
import torch

from dtmx.ops import functional as DF

CL = torch.channels_last


def nhwc(*shape):
    n = 1
    for s in shape:
        n *= s
    return torch.arange(n, dtype=torch.float32).reshape(shape).contiguous(
        memory_format=CL)


def test_cat_backward_gradient_has_the_strides_the_issue_names():
    """The premise: an NHWC gradient of (2,16,5,5) split in two by cat's
    backward is contiguous in neither format."""
    seen = []

    class Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, dy):
            seen.append((tuple(dy.shape), tuple(dy.stride())))
            return dy

    x = nhwc(2, 16, 5, 5).requires_grad_(True)
    y = torch.cat([Probe.apply(x[:, :8]), Probe.apply(x[:, 8:])], dim=1)
    y.backward(nhwc(2, 16, 5, 5))
    assert sorted(seen) == [((2, 8, 5, 5), (400, 1, 80, 16))] * 2


def test_is_dense():
    x = nhwc(2, 16, 5, 5)
    assert DF._is_dense(x)                               # NHWC
    assert DF._is_dense(x.contiguous())                  # NCHW
    assert DF._is_dense(x.contiguous().permute(3, 1, 0, 2))  # any dim order
    assert not DF._is_dense(x[:, :8])                    # channel slice: gaps
    assert not DF._is_dense(x.contiguous()[:, :8])
    assert not DF._is_dense(x[:, :, ::2])
    assert not DF._is_dense(x[:1].expand(2, 16, 5, 5))   # overlapping
    assert DF._is_dense(x[:1])                           # size-1 dim: any stride
    assert DF._is_dense(torch.zeros(8))
    assert DF._is_dense(nhwc(2, 16, 1, 1))


def test_dense_keeps_the_dim_order_of_a_slice():
    x = nhwc(2, 32, 5, 5)
    s = x[:, 8:24]
    assert s.stride() == (800, 1, 160, 32)
    d = DF._dense(s)
    assert d.is_contiguous(memory_format=CL) and d.stride() == (400, 1, 80, 16)
    assert torch.equal(d, s)
    assert DF._dense(x) is x                             # dense: no copy
    n = x.contiguous()[:, 8:24]
    assert DF._dense(n).is_contiguous()


@pytest.mark.parametrize("dy_kind", ["cat_narrow", "nchw", "nhwc", "2d_view"])
def test_gradient_is_brought_into_the_layout_of_y(dy_kind):
    y = nhwc(2, 8, 5, 5)
    if dy_kind == "cat_narrow":
        dy = nhwc(2, 16, 5, 5)[:, 8:]
        assert dy.stride() == (400, 1, 80, 16)
    elif dy_kind == "nchw":
        dy = nhwc(2, 8, 5, 5).contiguous()
    elif dy_kind == "2d_view":
        dy = torch.arange(400.).reshape(2, 200).view(2, 8, 5, 5)
    else:
        dy = nhwc(2, 8, 5, 5)
    out = DF._to_layout_of(dy, y)
    assert out.stride() == y.stride()
    assert torch.equal(out, dy)                          # same logical values
    if dy_kind == "nhwc":
        assert out is dy                                 # already there
    # and the other way round: y NCHW (relu fed by a linear layer's view)
    y2 = y.contiguous()
    out2 = DF._to_layout_of(dy, y2)
    assert out2.stride() == y2.stride() and torch.equal(out2, dy)


def test_layout_ignores_strides_of_size_one_dims():
    a = torch.zeros(2, 16, 1, 1)
    b = a.as_strided((2, 16, 1, 1), (16, 1, 16, 16))     # NHWC spelling
    assert b.is_contiguous(memory_format=CL) and a.stride() != b.stride()
    assert DF._same_layout(a, b) and DF._to_layout_of(a, b) is a


def test_same_layout_needs_same_shape():
    assert not DF._same_layout(torch.zeros(2, 8), torch.zeros(16))


def test_envelope():
    x = torch.zeros(2, 16, 5, 5, dtype=torch.bfloat16)
    assert DF._ew_in_envelope(x)
    assert DF._ew_in_envelope(x, x.clone())
    assert not DF._ew_in_envelope(torch.zeros(3, 5, 3, 3, dtype=torch.bfloat16))
    assert not DF._ew_in_envelope(torch.zeros(0, dtype=torch.bfloat16))
    assert not DF._ew_in_envelope(x, x.half())           # mixed dtypes
    assert not DF._ew_in_envelope(x, x[:1])              # broadcast


def test_cpu_path_unchanged():
    """On the CPU the ops are torch's; the cat graph gives torch's gradient."""
    torch.manual_seed(0)
    x = torch.randn(2, 16, 5, 5).contiguous(memory_format=CL)
    dy = torch.randn(2, 16, 5, 5).contiguous(memory_format=CL)
    grads = []
    for relu in (DF.relu, torch.relu):
        xi = x.clone().requires_grad_(True)
        y = torch.cat([relu(xi[:, :8]), relu(xi[:, 8:])], dim=1)
        y.backward(dy)
        grads.append(xi.grad)
    assert torch.equal(grads[0], grads[1])
    a = x.clone().requires_grad_(True)
    b = x.contiguous().clone().requires_grad_(True)
    DF.add_relu(a, b).backward(dy)
    assert torch.equal(a.grad, dy * (x > 0)) and torch.equal(b.grad, a.grad)
