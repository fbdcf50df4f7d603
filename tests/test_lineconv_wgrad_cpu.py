"""DF._lineconv_wgrad_in_envelope: the shapes lineconv_wgrad.hip accepts (the
predicate only looks at shapes, dtypes, layout and alignment, so CPU tensors
serve)."""
import pytest
import torch

from dtmx.ops import functional as DF


def _case(N, H, W, C, Ko, rs, dtype=torch.bfloat16):
    def cl(*s):
        return torch.zeros(s, dtype=dtype).contiguous(memory_format=torch.channels_last)

    return cl(N, C, H, W), cl(N, Ko, H, W), cl(Ko, C, *rs)


@pytest.mark.parametrize("shape,rs,stride,pad,want", [
    ((2, 17, 17, 192, 192), (1, 7), 1, (0, 3), True),
    ((2, 17, 17, 192, 192), (7, 1), 1, (3, 0), True),   # generic fwd, halo 102
    ((2, 8, 8, 448, 384), (3, 1), 1, (1, 0), True),
    ((1, 1, 44, 8, 8), (7, 1), 1, (3, 0), False),       # halo 264
    ((2, 17, 17, 192, 192), (1, 7), 2, (0, 3), False),  # stride
    ((2, 17, 17, 192, 192), (1, 7), 1, (0, 0), False),  # not same-padded
    ((2, 17, 17, 20, 192), (1, 7), 1, (0, 3), False),   # C % 8
    ((2, 17, 17, 192, 192), (3, 3), 1, (1, 1), False),  # not a line
    ((2, 17, 17, 192, 192), (1, 9), 1, (0, 4), False),  # T
])
def test_envelope(shape, rs, stride, pad, want):
    x, dy, w = _case(*shape, rs)
    assert DF._lineconv_wgrad_in_envelope(x, dy, w, stride, *pad) == want


def test_envelope_dy():
    x, dy, w = _case(2, 17, 17, 64, 64, (1, 7))
    assert DF._lineconv_wgrad_in_envelope(x, dy, w, 1, 0, 3)
    assert not DF._lineconv_wgrad_in_envelope(x, dy[:, :, :, :11], w, 1, 0, 3)
    assert not DF._lineconv_wgrad_in_envelope(x, dy.float(), w, 1, 0, 3)
