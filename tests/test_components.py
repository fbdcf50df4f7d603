"""Per-layer component tests (reference tests/python/unittest: test_optimizer,
test_io, test_metric, test_lr_scheduler, test_initializer subsets)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import dtmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from dtmx import initializer, lr_scheduler, metric
from dtmx.io import CSVIter, DataBatch, NDArrayIter, ResizeIter, SyntheticDataIter
from dtmx.optimizer import SGD, Adam, LBSGD, create as opt_create, get_updater


# ------------------------------------------------------------- optimizer

def test_sgd_momentum_reference_math():
    w = torch.ones(4)
    g = torch.full((4,), 2.0)
    opt = SGD(learning_rate=0.1, momentum=0.9, rescale_grad=0.5, wd=0.01)
    st = opt.create_state(0, w)
    opt.update(0, w, g, st)
    # g' = 2*0.5 + 0.01*1 = 1.01; mom = -0.1*1.01; w = 1 - 0.101
    assert torch.allclose(w, torch.full((4,), 1 - 0.101), atol=1e-6)
    opt.update(0, w, g, st)
    mom2 = 0.9 * -0.101 - 0.1 * (1.0 + 0.01 * w[0].item() + 0.0)
    # just sanity: momentum accumulates (larger step)
    assert w[0] < 1 - 2 * 0.101


def test_sgd_multi_precision_master_weights():
    w = torch.randn(8).bfloat16()
    opt = SGD(learning_rate=0.1, momentum=0.9, multi_precision=True)
    st = opt.create_state_multi_precision(0, w)
    master, _ = st
    assert master.dtype == torch.float32
    g = torch.randn(8).bfloat16()
    opt.update_multi_precision(0, w, g, st)
    assert torch.allclose(w.float(), master, atol=0.01)


def test_adam_step():
    w = torch.ones(4)
    opt = Adam(learning_rate=0.01)
    st = opt.create_state(0, w)
    opt.update(0, w, torch.ones(4), st)
    assert (w < 1).all()


def test_clip_gradient():
    w = torch.zeros(2)
    opt = SGD(learning_rate=1.0, clip_gradient=0.1)
    opt.update(0, w, torch.tensor([10.0, -10.0]), None)
    assert torch.allclose(w, torch.tensor([-0.1, 0.1]))


def test_create_registry():
    assert isinstance(opt_create("sgd"), SGD)
    assert isinstance(opt_create("adam"), Adam)
    assert isinstance(opt_create("lbsgd"), LBSGD)


def test_updater_state_per_index():
    opt = SGD(learning_rate=0.1, momentum=0.9)
    upd = get_updater(opt)
    w0, w1 = torch.ones(2), torch.ones(3)
    upd(0, torch.ones(2), w0)
    upd(1, torch.ones(3), w1)
    assert set(upd.get_states().keys()) == {0, 1}


# ------------------------------------------------------------------- io

def test_ndarrayiter_sharding():
    data = np.arange(100, dtype=np.float32).reshape(100, 1)
    it0 = NDArrayIter({"data": data}, batch_size=10, part_index=0, num_parts=2,
                      shuffle=False)
    it1 = NDArrayIter({"data": data}, batch_size=10, part_index=1, num_parts=2,
                      shuffle=False)
    b0 = it0.next().data[0]
    b1 = it1.next().data[0]
    assert b0[0, 0] == 0 and b1[0, 0] == 50  # disjoint shards


def test_ndarrayiter_pad_last_batch():
    data = np.arange(25, dtype=np.float32).reshape(25, 1)
    it = NDArrayIter({"data": data}, batch_size=10, shuffle=False)
    batches = list(it)
    assert len(batches) == 3
    assert batches[2].pad == 5


def test_resize_iter_caps_epoch():
    it = ResizeIter(SyntheticDataIter(10, (4, 8), max_iter=100), size=7)
    assert len(list(it)) == 7
    it.reset()
    assert len(list(it)) == 7


def test_csv_iter(tmp_path):
    f = str(tmp_path / "d.csv")
    np.savetxt(f, np.arange(12).reshape(4, 3), delimiter=",")
    lf = str(tmp_path / "l.csv")
    np.savetxt(lf, np.arange(4), delimiter=",")
    it = CSVIter(f, (3,), lf, batch_size=2)
    b = it.next()
    assert b.data[0].shape == (2, 3)


# --------------------------------------------------------------- metric

def test_accuracy_and_topk():
    preds = torch.tensor([[0.1, 0.9], [0.8, 0.2]])
    labels = torch.tensor([1.0, 1.0])
    acc = metric.create("acc")
    acc.update([labels], [preds])
    assert dict(acc.get_name_value())["accuracy"] == 0.5
    topk = metric.TopKAccuracy(2)
    topk.update([labels], [preds])
    assert dict(topk.get_name_value())["top_k_accuracy_2"] == 1.0


def test_composite_metric():
    m = metric.create(["acc", "ce"])
    preds = torch.tensor([[0.2, 0.8]])
    m.update([torch.tensor([1.0])], [preds])
    names, values = m.get()
    assert "accuracy" in names and "cross-entropy" in names


def test_metric_tail_vs_closed_forms():
    """F1/MCC/MAE/MSE/RMSE/Perplexity/Pearson vs hand-computed values
    (reference metric.py:605-1263 classes)."""
    import math

    labels = torch.tensor([1.0, 0.0, 1.0, 0.0])
    preds = torch.tensor([[0.2, 0.8], [0.3, 0.7], [0.9, 0.1], [0.6, 0.4]])
    # pred labels: 1, 1, 0, 0 -> tp=1 fp=1 tn=1 fn=1
    f1 = metric.create("f1")
    f1.update([labels], [preds])
    assert abs(dict(f1.get_name_value())["f1"] - 0.5) < 1e-9
    mcc = metric.create("mcc")
    mcc.update([labels], [preds])
    assert abs(dict(mcc.get_name_value())["mcc"] - 0.0) < 1e-9

    y = torch.tensor([[1.0, 2.0, 3.0]])
    p = torch.tensor([[2.0, 2.0, 5.0]])
    mae = metric.create("mae")
    mae.update([y], [p])
    assert abs(mae.get()[1] - 1.0) < 1e-6
    mse = metric.create("mse")
    mse.update([y], [p])
    assert abs(mse.get()[1] - 5.0 / 3) < 1e-6
    rmse = metric.create("rmse")
    rmse.update([y], [p])
    assert abs(rmse.get()[1] - math.sqrt(5.0 / 3)) < 1e-6

    probs = torch.tensor([[0.5, 0.5], [0.25, 0.75]])
    lab = torch.tensor([0.0, 1.0])
    ppl = metric.create("perplexity")
    ppl.update([lab], [probs])
    expect = math.exp(-(math.log(0.5) + math.log(0.75)) / 2)
    assert abs(ppl.get()[1] - expect) < 1e-6
    # ignore_label drops the masked row
    ppl2 = metric.Perplexity(ignore_label=0)
    ppl2.update([lab], [probs])
    assert abs(ppl2.get()[1] - math.exp(-math.log(0.75))) < 1e-6

    pr = metric.create("pearsonr")
    pr.update([torch.tensor([1.0, 2.0, 3.0])], [torch.tensor([2.0, 4.0, 6.0])])
    assert abs(pr.get()[1] - 1.0) < 1e-6

    nll = metric.create("nll_loss")
    nll.update([lab], [probs])
    assert abs(nll.get()[1] + (math.log(0.5) + math.log(0.75)) / 2) < 1e-6


def test_custom_metric_and_np():
    def feval(label, pred):
        return float((label == pred.argmax(-1)).mean())

    m = metric.np(feval, name="myacc")
    m.update([torch.tensor([1, 0])], [torch.tensor([[0.1, 0.9], [0.2, 0.8]])])
    assert abs(m.get()[1] - 0.5) < 1e-9
    assert "myacc" in m.name


# ---------------------------------------------------------- lr scheduler

def test_multifactor():
    s = lr_scheduler.MultiFactorScheduler([10, 20], factor=0.1)
    s.base_lr = 1.0
    assert s(5) == 1.0
    assert s(15) == pytest.approx(0.1)
    assert s(25) == pytest.approx(0.01)


def test_warmup_rearm():
    s = lr_scheduler.WarmupScheduler(1.0, warmup_steps=10)
    assert s(0) == 0.0
    assert s(5) == pytest.approx(0.5)
    assert s(10) == 1.0
    s.rearm(100)  # worker join: ramp again (dynamic minibatch paper)
    assert s(105) == pytest.approx(0.5)


def test_cosine_scheduler():
    s = lr_scheduler.CosineScheduler(max_update=100, base_lr=1.0, final_lr=0.1)
    assert s(0) == pytest.approx(1.0)
    assert s(50) == pytest.approx(0.55)   # midpoint = (1.0+0.1)/2
    assert s(100) == pytest.approx(0.1)
    assert s(150) == pytest.approx(0.1)   # clamped after max_update


# ----------------------------------------------------------- initializer

def test_xavier_scale():
    w = torch.empty(64, 64)
    initializer.Xavier(rnd_type="uniform", factor_type="avg", magnitude=3)("fc_weight", w)
    bound = math.sqrt(3.0 / 64)
    assert w.abs().max() <= bound + 1e-6


def test_name_based_dispatch():
    ini = initializer.create("default")
    b = torch.randn(4)
    ini("fc1_bias", b)
    assert torch.equal(b, torch.zeros(4))
    g = torch.randn(4)
    ini("bn0_gamma", g)
    assert torch.equal(g, torch.ones(4))


def test_initializer_tail():
    """Constant/Orthogonal/Bilinear/LSTMBias/Mixed (reference
    initializer.py:287-702)."""
    w = torch.empty(3, 5)
    initializer.Constant(0.5)("w_weight", w)
    assert torch.equal(w, torch.full((3, 5), 0.5))

    q = torch.empty(16, 32)
    initializer.Orthogonal(scale=1.0, rand_type="gaussian")("w_weight", q)
    eye = q.float() @ q.float().T
    assert torch.allclose(eye, torch.eye(16), atol=1e-4)

    d = torch.empty(2, 1, 4, 4)
    initializer.Bilinear()("deconv_weight", d)
    # bilinear kernel: symmetric, peak at the center block
    assert d[0, 0, 1, 1] == d[0, 0, 2, 2] == d.max()
    assert torch.allclose(d[0, 0], d[0, 0].flip(0).flip(1))

    b = torch.empty(16)
    initializer.LSTMBias(forget_bias=1.0)("lstm_i2h_bias", b)
    assert b[4:8].eq(1).all() and b[:4].eq(0).all() and b[8:].eq(0).all()

    mixed = initializer.Mixed([".*bias", ".*"],
                              [initializer.Zero(), initializer.One()])
    t1, t2 = torch.randn(3), torch.randn(3)
    mixed("fc_bias", t1)
    mixed("fc_weight", t2)
    assert t1.eq(0).all() and t2.eq(1).all()


# ----------------------------------------------------- optimizer states io

def test_kvstore_optimizer_states_roundtrip(tmp_path):
    kv = dtmx.kvstore.create("local")
    kv.set_optimizer(SGD(learning_rate=0.1, momentum=0.9))
    kv.init("w", torch.ones(4))
    kv.push("w", torch.ones(4))
    f = str(tmp_path / "opt.states")
    kv.save_optimizer_states(f)
    kv2 = dtmx.kvstore.create("local")
    kv2.set_optimizer(SGD(learning_rate=0.1, momentum=0.9))
    kv2.load_optimizer_states(f)
    s1 = kv._updater.get_states()
    s2 = kv2._updater.get_states()
    assert set(s1) == set(s2)
    for k in s1:
        assert torch.allclose(s1[k], s2[k])


# --------------------------------------------------- test_utils + row_sparse

def test_check_numeric_gradient_harness():
    from dtmx.test_utils import check_numeric_gradient

    w = torch.randn(3, 3)
    check_numeric_gradient(lambda t: (t * t).sum(), [w])


def test_row_sparse_pull():
    kv = dtmx.kvstore.create("local")
    kv.init("emb", torch.arange(20, dtype=torch.float32).reshape(5, 4))
    out = torch.zeros(5, 4)
    kv.row_sparse_pull("emb", out=out, row_ids=torch.tensor([1, 3]))
    assert out[1, 0] == 4 and out[3, 3] == 15
    assert out[0].sum() == 0 and out[2].sum() == 0


def test_speedometer_and_checkpoint_callbacks(tmp_path, caplog):
    import logging

    import dtmx

    from dtmx.callback import BatchEndParam, Speedometer, do_checkpoint
    from dtmx.io import DataBatch
    from dtmx.models import get_symbol

    net = get_symbol("mlp", num_classes=10, input_dim=16)
    mod = dtmx.Module(net, context=dtmx.cpu())
    mod.bind(data_shapes=[("data", (4, 16))], label_shapes=[("softmax_label", (4,))])
    mod.init_params()
    mod.init_optimizer()
    batch = DataBatch(data=[torch.randn(4, 16)], label=[torch.randint(0, 10, (4,)).float()])
    mod.forward_backward(batch)
    mod.update()

    speed = Speedometer(batch_size=4, frequent=2)
    with caplog.at_level(logging.INFO):
        for nb in range(5):
            speed(BatchEndParam(epoch=0, nbatch=nb, eval_metric=None, locals=None))
    assert any("samples/sec" in r.message for r in caplog.records)

    cb = do_checkpoint(str(tmp_path / "ck"), period=1)
    cb(0, mod.symbol, *mod.get_params())
    assert (tmp_path / "ck-0001.params").exists()
    _sym, arg, aux = dtmx.model.load_checkpoint(str(tmp_path / "ck"), 1)
    assert set(arg) == {n for n, _ in net.named_parameters()}


def test_callback_tail(tmp_path, caplog):
    """module_checkpoint / log_train_metric / ProgressBar (reference
    callback.py:27-117,184-212)."""
    import logging

    from dtmx import callback

    class FakeMod:
        saved = None

        def save_checkpoint(self, prefix, epoch, save_optimizer_states=False):
            FakeMod.saved = (prefix, epoch, save_optimizer_states)

    cb = callback.module_checkpoint(FakeMod(), str(tmp_path / "m"), period=2,
                                    save_optimizer_states=True)
    cb(0)
    assert FakeMod.saved is None  # epoch 1: not on period
    cb(1)
    assert FakeMod.saved == (str(tmp_path / "m"), 2, True)

    m = metric.create("acc")
    m.update([torch.tensor([1.0])], [torch.tensor([[0.1, 0.9]])])
    with caplog.at_level(logging.INFO):
        callback.log_train_metric(5, auto_reset=True)(
            callback.BatchEndParam(epoch=0, nbatch=5, eval_metric=m))
    assert any("Train-accuracy" in r.getMessage() for r in caplog.records)
    assert m.num_inst == 0  # auto_reset

    callback.ProgressBar(total=10, length=10)(
        callback.BatchEndParam(epoch=0, nbatch=5, eval_metric=None))


def test_monitor_collects_stats():
    import dtmx

    from dtmx.io import DataBatch
    from dtmx.models import get_symbol
    from dtmx.monitor import Monitor

    net = get_symbol("mlp", num_classes=10, input_dim=16)
    mod = dtmx.Module(net, context=dtmx.cpu())
    mod.bind(data_shapes=[("data", (4, 16))], label_shapes=[("softmax_label", (4,))])
    mod.init_params()
    mod.init_optimizer()
    mon = Monitor(interval=1)
    mon.install(mod)
    batch = DataBatch(data=[torch.randn(4, 16)], label=[torch.randint(0, 10, (4,)).float()])
    mon.tic()
    mod.forward_backward(batch)
    rows = mon.toc()
    assert rows and all(len(r) == 3 for r in rows)
    assert any(name.endswith("_grad") for _, name, _ in rows)


def test_profiler_chrome_trace(tmp_path):
    from dtmx import profiler

    out = str(tmp_path / "trace.json")
    profiler.set_config(filename=out)
    profiler.set_state("run")
    torch.randn(32, 32) @ torch.randn(32, 32)
    profiler.set_state("stop")
    assert os.path.exists(out) and os.path.getsize(out) > 100


def test_gluon_trainer_step():
    from dtmx import gluon

    net = torch.nn.Linear(8, 4)
    trainer = gluon.Trainer(net.parameters(), "sgd",
                            {"learning_rate": 0.5}, kvstore="local")
    x = torch.randn(16, 8)
    w0 = net.weight.detach().clone()
    loss = gluon.L2Loss()(net(x), torch.zeros(16, 4)).mean()
    loss.backward()
    trainer.step(batch_size=16)
    assert not torch.allclose(net.weight.detach(), w0)


def test_prefetching_iter():
    from dtmx.io import PrefetchingIter

    base = SyntheticDataIter(10, (4, 8), max_iter=6)
    it = PrefetchingIter(base)
    b1 = list(it)
    assert len(b1) == 6
    it.reset()
    b2 = list(it)
    assert len(b2) == 6
    assert it.provide_data == base.provide_data


def test_mnist_iter_synthetic_fallback(tmp_path):
    from dtmx.io import MNISTIter

    it = MNISTIter(image=str(tmp_path / "none"), label=str(tmp_path / "nol"),
                   batch_size=32)
    b = it.next()
    assert b.data[0].shape == (32, 1, 28, 28)
    assert b.label[0].shape == (32,)


# ----------------------------------------------------- cluster tools tail

def test_parse_log(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import parse_log

    lines = [
        "INFO Epoch[0] Train-accuracy=0.512000\n",
        "INFO Epoch[0] Time cost=12.345\n",
        "INFO Epoch[0] Validation-accuracy=0.423000\n",
        "INFO Epoch[1] Train-accuracy=0.734000\n",
        "INFO Epoch[1] Time cost=11.002\n",
    ]
    rows = parse_log.parse(lines)
    assert rows[0]["train-accuracy"] == 0.512
    assert rows[0]["valid-accuracy"] == 0.423
    assert rows[1]["time"] == 11.002
    md = parse_log.to_markdown(rows)
    assert md.count("|") > 10 and "0.734" in md


def test_kill_dtmx_pidfiles(tmp_path):
    import subprocess
    import sys as _sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kill_dtmx

    rundir = tmp_path / "run"
    rundir.mkdir()
    p = subprocess.Popen([_sys.executable, "-c", "import time; time.sleep(60)"])
    (rundir / "127.0.0.1#0.pid").write_text(str(p.pid))
    (rundir / "stale.pid").write_text("999999")  # no such pid: skipped
    n = kill_dtmx.kill_local(str(rundir))
    assert n == 1
    assert p.wait(timeout=15) != 0  # SIGTERM'd
    assert not list(rundir.glob("*.pid"))  # ledger cleaned


def test_gluon_trainer_state_roundtrip(tmp_path):
    import dtmx.gluon as gluon
    from dtmx.models import get_symbol

    net = get_symbol("mlp", num_classes=10, input_dim=16)
    tr = gluon.Trainer(net.parameters(), "sgd",
                       {"learning_rate": 0.1, "momentum": 0.9})
    x = torch.randn(4, 16)
    out = net(x)
    out.sum().backward()
    tr.step(batch_size=4)
    f = str(tmp_path / "t.states")
    tr.save_states(f)
    tr2 = gluon.Trainer(net.parameters(), "sgd",
                        {"learning_rate": 0.1, "momentum": 0.9})
    tr2.load_states(f)
    s1 = tr._updater.get_states()
    s2 = tr2._updater.get_states()
    assert set(s1) == set(s2)
    for k in s1:
        a = s1[k][0] if isinstance(s1[k], tuple) else s1[k]
        b = s2[k][0] if isinstance(s2[k], tuple) else s2[k]
        if a is not None:
            torch.testing.assert_close(a.cpu(), b.cpu())


def test_bench_json_contract(tmp_path):
    """bench.py emits exactly one driver-consumable JSON line with the
    contract fields (BASELINE.json metric/config names)."""
    import json as _json
    import subprocess
    import sys as _sys

    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(
        [_sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1",
         "--warmup", "0", "--batch-size", "4"],
        capture_output=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = _json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
              "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config"):
        assert k in d, k
    assert d["metric"].startswith("images/sec ResNet-50")
    assert d["data"] == "synthetic"
    assert d["scaling"] == "weak"
    assert d["config"]["model"] == "resnet-50"
    assert d["config"]["global_batch"] == 4
    assert d["config"]["parallelism"] == "dp1"


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes one step of the timed path, taken from the
    seeded pre-warmup state, as float .npy files (<= 64 MB in all): the dump
    is the same from run to run, whatever --steps/--warmup/--full ran before
    it (CPU run, so bit for bit)."""
    import json as _json
    import subprocess
    import sys as _sys

    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)

    def run(name, steps, warmup, *extra):
        out = tmp_path / name
        r = subprocess.run(
            [_sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
             "--steps", str(steps), "--warmup", str(warmup),
             "--batch-size", "4", "--num-layers", "18",
             "--image-shape", "3,32,32", "--dump-outputs", str(out), *extra],
            capture_output=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        d = _json.loads(lines[0])
        arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
        return d, arrays

    d1, a1 = run("a", 1, 0)
    d2, a2 = run("b", 3, 2, "--full")
    assert (d1["steps"], d1["warmup"]) == (1, 0)
    assert (d2["steps"], d2["warmup"]) == (3, 2)
    assert d1["ms_per_step"] > 0 and d2["ms_per_step"] > 0
    assert set(a1) == set(a2) == {"loss", "logits", "params_sample", "aux_stats"}
    assert a1["logits"].shape == (4, 1000)
    assert sum(a.nbytes for a in a1.values()) <= 64 << 20
    for k, a in a1.items():
        assert a.dtype in (np.float32, np.float64), (k, a.dtype)
        assert np.isfinite(a).all(), k
        np.testing.assert_array_equal(a, a2[k], err_msg=k)


def test_bench_dist_contract_world2(tmp_path):
    """bench.py under the driver's multi-rank launch pattern (torchrun env:
    RANK/WORLD_SIZE/LOCAL_RANK/MASTER_*), world 2 on gloo/CPU: both ranks
    finish, rank 0 prints ONE whole-job JSON line with n_gpus=2 — de-risks
    the round-end 8-GPU scaling run."""
    import json as _json
    import socket
    import subprocess
    import sys as _sys

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for rank in range(2):
        env = dict(os.environ)
        env.update(RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   DTMX_BACKEND="gloo", DTMX_BENCH_AUX="0")
        procs.append(subprocess.Popen(
            [_sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2",
             "--steps", "1", "--warmup", "0", "--batch-size", "4"],
            stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env))
    outs = []
    for p in procs:
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, err.decode()[-2000:]
        outs.append(out.decode())
    json_lines = [ln for o in outs for ln in o.splitlines() if ln.startswith("{")]
    assert len(json_lines) == 1, json_lines  # rank 0 only
    d = _json.loads(json_lines[0])
    assert d["n_gpus"] == 2
    assert d["config"]["parallelism"] == "dp2"
    assert d["config"]["global_batch"] == 8  # whole-job aggregate


def test_gluon_namespaces():
    """gluon.nn / gluon.loss / gluon.data map gluon ctor idioms onto the
    substrate (reference gluon/nn, gluon/loss, gluon/data)."""
    from dtmx import gluon

    net = gluon.nn.Sequential(
        gluon.nn.Dense(8, in_units=4, activation="relu"),
        gluon.nn.Dense(2, in_units=8))
    y = net(torch.randn(3, 4))
    assert y.shape == (3, 2)
    conv = gluon.nn.Conv2D(6, 3, in_channels=2, padding=1)
    assert conv(torch.randn(1, 2, 5, 5)).shape == (1, 6, 5, 5)
    assert gluon.nn.MaxPool2D(2)(torch.randn(1, 2, 4, 4)).shape == (1, 2, 2, 2)
    losses = gluon.loss.SoftmaxCrossEntropyLoss()(y, torch.tensor([0, 1, 0]))
    assert losses.shape == (3,)
    assert gluon.loss.L1Loss()(y, torch.zeros(3, 2)).shape == (3, 2)
    ds = gluon.data.ArrayDataset(torch.randn(10, 4), torch.arange(10))
    dl = gluon.data.DataLoader(ds, batch_size=5)
    assert len(list(dl)) == 2
    # Block/HybridBlock are nn.Module aliases
    assert gluon.Block is torch.nn.Module


def test_symbol_stub_and_lrn_fallback():
    """dtmx.symbol raises with directions (no symbolic layer by design);
    LRN's CPU path matches torch's reference op."""
    import pytest as _pytest
    import torch.nn.functional as F

    import dtmx
    from dtmx.ops.layers import LRN

    with _pytest.raises(AttributeError, match="no symbolic graph"):
        dtmx.symbol.Variable("data")
    x = torch.randn(2, 16, 5, 5)
    torch.testing.assert_close(LRN()(x),
                               F.local_response_norm(x, 5, 1e-4, 0.75, 2.0))


def test_random_api():
    import dtmx.random as rnd

    rnd.seed(42)
    a = rnd.uniform(0, 1, (4, 4))
    rnd.seed(42)
    b = rnd.uniform(0, 1, (4, 4))
    torch.testing.assert_close(a, b)
    n = rnd.normal(0, 2, (1000,))
    assert abs(n.std().item() - 2.0) < 0.3
    r = rnd.randint(0, 10, (100,))
    assert r.min() >= 0 and r.max() < 10


def test_rnn_layer_shapes_and_training():
    from dtmx.rnn import RNNLayer

    for mode in ("lstm", "gru", "rnn_tanh"):
        layer = RNNLayer(hidden_size=8, num_layers=2, mode=mode,
                         input_size=6)
        x = torch.randn(5, 3, 6)  # (T, N, C)
        st = layer.begin_state(3)
        out, st2 = layer(x, st if mode == "lstm" else st[0])
        assert out.shape == (5, 3, 8)
        out.sum().backward()
        assert next(layer.parameters()).grad is not None


def test_image_api_roundtrip():
    import numpy as np

    import dtmx.image as img
    from dtmx.ops.hip import require_ext

    ext = require_ext()
    ys, xs = np.mgrid[0:20, 0:24]
    im = np.stack([ys * 5 % 256, xs * 7 % 256, (ys + xs) % 256],
                  axis=-1).astype(np.uint8)
    enc = ext.encode_jpeg(im.tobytes(), 20, 24, 3, 95)
    dec = img.imdecode(bytes(enc))
    assert tuple(dec.shape) == (20, 24, 3)
    small = img.resize_short(dec, 10)
    assert min(small.shape[0], small.shape[1]) == 10
    crop, (x0, y0, tw, th) = img.center_crop(dec, (10, 12))
    assert tuple(crop.shape) == (10, 12, 3) and (x0, y0) == (6, 5)
    rc, _ = img.random_crop(dec, (8, 8))
    assert tuple(rc.shape) == (8, 8, 3)
    flipped = img.horizontal_flip(dec)
    assert torch.equal(flipped[:, 0], dec[:, -1])


def test_print_summary():
    from dtmx.models import get_symbol
    from dtmx.visualization import print_summary

    net = get_symbol("mlp", num_classes=10, input_dim=16)
    text = print_summary(net, shape=(2, 16))
    assert "Total params" in text and "Linear" in text
