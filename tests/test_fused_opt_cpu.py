"""Host side of the fused flat-bucket NAG / LBSGD steps: the segment and chunk
tables, the routing in Module.init_optimizer without a GPU, and the warmup
learning rate shared by LBSGD.update and the fused path."""
import math

import pytest
import torch

import dtmx
from dtmx import Module, cpu
from dtmx.io import NDArrayIter
from dtmx.models import get_symbol
from dtmx.optimizer.optimizer import LBSGD
from dtmx.parallel.bucketer import OPT_CHUNK, build_segment_tables

CHUNK = OPT_CHUNK
SIZES = [1, 7, 8, 9, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]


def test_chunk_constant():
    assert 1024 <= CHUNK <= 8192 and CHUNK & (CHUNK - 1) == 0


@pytest.mark.parametrize("sizes", [SIZES, SIZES[::-1], [5], [0, 3, 0, CHUNK + 2, 0]],
                         ids=["issue", "reversed", "one", "empty-segments"])
def test_segment_tables(sizes):
    t = build_segment_tables(sizes, CHUNK)
    seg_off, cseg, cstart, clen, sco = (t[k] for k in (
        "seg_off", "chunk_seg", "chunk_start", "chunk_len", "seg_chunk_off"))
    total = sum(sizes)
    assert seg_off[0] == 0 and seg_off[-1] == total
    assert [b - a for a, b in zip(seg_off, seg_off[1:])] == list(sizes)
    assert len(cseg) == len(cstart) == len(clen)
    assert len(sco) == len(sizes) + 1 and sco[0] == 0 and sco[-1] == len(cseg)

    # every element is covered by exactly one chunk
    cover = [0] * total
    for s, st, ln in zip(cseg, cstart, clen):
        assert 1 <= ln <= CHUNK
        # no chunk straddles a segment
        assert seg_off[s] <= st and st + ln <= seg_off[s + 1]
        for i in range(st, st + ln):
            cover[i] += 1
    assert cover == [1] * total

    for s, n in enumerate(sizes):
        # the chunks of a segment are consecutive and in order ...
        mine = [c for c in range(len(cseg)) if cseg[c] == s]
        assert mine == list(range(sco[s], sco[s + 1]))
        assert len(mine) == -(-n // CHUNK)
        # ... and counted from the segment's start: chunk k starts at k * CHUNK
        # and all but the last are full
        for k, c in enumerate(mine):
            assert cstart[c] - seg_off[s] == k * CHUNK
            assert clen[c] == min(CHUNK, n - k * CHUNK)


def test_segment_tables_independent_of_placement():
    """A parameter's chunking depends on its own size only."""
    def rel(sizes, s):
        t = build_segment_tables(sizes, CHUNK)
        return [(t["chunk_start"][c] - t["seg_off"][s], t["chunk_len"][c])
                for c in range(len(t["chunk_seg"])) if t["chunk_seg"][c] == s]
    n = 3 * CHUNK + 5
    assert rel([n], 0) == rel([1, 7, n, 9], 2) == rel([CHUNK - 1, n], 1)


# ------------------------------------------------------------- routing on CPU

def _mlp(optimizer, **params):
    torch.manual_seed(0)
    net = get_symbol("mlp", num_classes=10, input_dim=16)
    mod = Module(net, context=cpu())
    mod.bind(data_shapes=[("data", (8, 16))], label_shapes=[("softmax_label", (8,))])
    mod.init_params()
    p = dict(learning_rate=0.1, momentum=0.9, wd=1e-4)
    p.update(params)
    mod.init_optimizer(optimizer=optimizer, optimizer_params=tuple(p.items()))
    return mod


@pytest.mark.parametrize("name", ["lbsgd", "nag", "sgd"])
def test_cpu_stays_per_tensor_and_trains(name):
    mod = _mlp(name)
    assert mod._use_fused_sgd is False and mod._fused_kind is None
    g = torch.Generator().manual_seed(1)
    X = torch.randn(8, 16, generator=g)
    Y = torch.randint(0, 10, (8,), generator=g).float()
    batch = next(iter(NDArrayIter({"data": X}, {"softmax_label": Y}, 8)))
    losses = []
    for _ in range(3):
        before = [p.detach().clone() for p in mod.symbol.parameters()]
        mod.forward_backward(batch)
        losses.append(mod._loss.item())
        mod.update()
        assert any(not torch.equal(b, a)
                   for b, a in zip(before, mod.symbol.parameters()))
    assert mod._optimizer.num_update == 3
    assert all(math.isfinite(v) for v in losses)
    if name != "lbsgd":      # lbsgd's trust ratio makes three steps tiny
        assert losses[-1] < losses[0], losses


# -------------------------------------------------------------------- warmup

# sum of the three weights (exact in fp64) after each of eight LBSGD.update
# calls, recorded from the code as it was before warmup_lr was factored out.
RECORDED = {
    ("linear", 0.02): ['0x1.1030bd0000000p+0', '0x1.10a5a88000000p+0', '0x1.116fff8000000p+0', '0x1.129eda0000000p+0', '0x1.143f290000000p+0', '0x1.1643ff0000000p+0', '0x1.18a1604000000p+0', '0x1.1b4c3fc000000p+0'],
    ("linear", 1000.0): ['0x1.1332820000000p+0', '0x1.1fabb50000000p+0', '0x1.3e174e8000000p+0', '0x1.79761c0000000p+0', '0x1.dee2240000000p+0', '0x1.39dfd80000000p+1', '0x1.9e74560000000p+1', '0x1.0fae9b0000000p+2'],
    ("sqrt", 0.02): ['0x1.10546b8000000p+0', '0x1.11079c0000000p+0', '0x1.121f820000000p+0', '0x1.139f118000000p+0', '0x1.1587090000000p+0', '0x1.17cb210000000p+0', '0x1.1a60038000000p+0', '0x1.1d3b3fc000000p+0'],
    ("sqrt", 1000.0): ['0x1.1589af8000000p+0', '0x1.2817ab8000000p+0', '0x1.504ca98000000p+0', '0x1.9787e10000000p+0', '0x1.03d0380000000p+1', '0x1.530c7d8000000p+1', '0x1.bbf3500000000p+1', '0x1.205fd18000000p+2'],
    ("none", 0.02): ['0x1.1092368000000p+0', '0x1.11a7850000000p+0', '0x1.1331c48000000p+0', '0x1.1523c20000000p+0', '0x1.17713f0000000p+0', '0x1.1a0ee78000000p+0', '0x1.1cf2510000000p+0', '0x1.2011f20000000p+0'],
    ("none", 1000.0): ['0x1.1997838000000p+0', '0x1.356a82c000000p+0', '0x1.6b3fa20000000p+0', '0x1.c216420000000p+0', '0x1.201d2bc000000p+1', '0x1.75ab324000000p+1', '0x1.e441c00000000p+1', '0x1.3715f90000000p+2'],
}


def _lbsgd(strategy, eta, **kw):
    return LBSGD(momentum=0.9, learning_rate=0.3, wd=1e-4,
                 warmup_strategy=strategy, warmup_epochs=2, updates_per_epoch=3,
                 eta=eta, rescale_grad=0.5, **kw)


@pytest.mark.parametrize("strategy,eta", sorted(RECORDED))
def test_lbsgd_update_unchanged(strategy, eta):
    """warmup_updates is 6: steps 1-5 ramp, steps 6-8 do not."""
    opt = _lbsgd(strategy, eta)
    w = torch.tensor([1.5, -0.75, 0.3125])
    st = opt.create_state(0, w)
    got = []
    for step in range(8):
        opt.update(0, w, torch.tensor([0.25, -1.0, 0.5]) * (step + 1), st)
        got.append(w.double().sum().item().hex())
    assert got == RECORDED[(strategy, eta)]


def test_warmup_lr_values():
    for strategy in ("linear", "sqrt", "none"):
        opt = _lbsgd(strategy, 0.02)
        assert opt.warmup_updates == 6
        for t in range(1, 9):
            want = 0.3
            if t < 6 and strategy == "linear":
                want = 0.3 * (t + 1) / 6
            elif t < 6 and strategy == "sqrt":
                want = 0.3 * math.sqrt((t + 1) / 6)
            assert opt.warmup_lr(0.3, t) == want


class _FakeBucketer:
    async_mode = False

    def __init__(self):
        self.calls = []

    def finish(self):
        pass

    def fused_lbsgd_step(self, lr, momentum, wd, rescale, clip, eta, hyper=None):
        self.calls.append((lr, momentum, wd, rescale, clip, eta, hyper))


@pytest.mark.parametrize("scheduler", [False, True])
@pytest.mark.parametrize("strategy", ["linear", "sqrt", "none"])
def test_fused_lr_is_update_lr(strategy, scheduler):
    """Module.update's lbsgd branch hands fused_lbsgd_step the lr that
    LBSGD.update computes at the same step (same scheduler, same ramp)."""
    from dtmx.lr_scheduler import FactorScheduler

    def sched():
        return FactorScheduler(step=2, factor=0.5) if scheduler else None

    # per-tensor: record the lr update() ends up with, via the shared helper
    ref = _lbsgd(strategy, 0.02, lr_scheduler=sched())
    used = []
    orig = ref.warmup_lr
    ref.warmup_lr = lambda lr, t: used.append(orig(lr, t)) or used[-1]
    w = torch.tensor([1.5, -0.75, 0.3125])
    st = ref.create_state(0, w)
    for _ in range(8):
        ref.update(0, w, torch.tensor([0.25, -1.0, 0.5]), st)

    mod = _mlp("sgd")
    mod._optimizer = _lbsgd(strategy, 0.02, lr_scheduler=sched(), clip_gradient=2.0)
    mod._bucketer = fake = _FakeBucketer()
    mod._use_fused_sgd, mod._fused_kind = True, "lbsgd"
    for _ in range(8):
        mod.update()
    assert mod._optimizer.num_update == 8
    assert [c[0] for c in fake.calls] == used
    assert fake.calls[0][1:] == (0.9, 1e-4, 0.5, 2.0, 0.02, None)
