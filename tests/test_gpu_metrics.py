"""Clip evaluation on the MI355X: the ww_clip_metrics record against the numpy restatement (tests/metrics_ref.py) integer for integer,
and the callers -- WakewordTrainer.validate / val_report / monitor= and inference.evaluate_report -- against the logits they ran on."""
import numpy as np
import pytest
import torch

import metrics_ref as ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import inference, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
THRESHOLDS = (0.5, 0.8, 0.999)


def _feed(state, z, y, sizes=None):
    """Logits [n, 2] and labels [n] (numpy) into the record, whole or in calls of the given sizes."""
    zt, yt = torch.from_numpy(np.ascontiguousarray(z, np.float32)).to(DEV), torch.from_numpy(np.ascontiguousarray(y, np.int64)).to(DEV)
    n, calls, s = len(y), 0, 0
    sizes = sizes or [n]
    while s < n:
        for b in sizes:
            if s >= n:
                break
            ops.clip_metrics_update(zt[s:s + b], yt[s:s + b], state)
            calls += 1
            s += b
    return calls


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 4097])
def test_counters_equal_the_restatement(n):
    rng = np.random.default_rng(100 + n)
    z = (rng.standard_normal((n, 2)) * 30.0).astype(np.float32)            # margins of spread 42: about 45 % pass +-32
    y = (rng.random(n) < 0.12).astype(np.int64)                           # imbalanced
    state = ops.new_clip_metrics(DEV, THRESHOLDS)
    assert _feed(state, z, y) == 1
    r = ops.read_clip_metrics(state)
    want = ref.counters(z, y, state.margins)
    d = ref.margins_of(z)
    if n >= 1000:
        assert (d >= 32).any() and (d < -32).any() and want["hist"][:, 0].sum() > 0 and want["hist"][:, -1].sum() > 0
    ref.assert_counters(r, want, batches=1)
    assert r.thresholds == THRESHOLDS and np.array_equal(r.margins, [nat.lib.ww_clip_metrics_margin_host(p) for p in THRESHOLDS])
    assert r.total == n and r.confusion.sum() == n and r.hist.sum() == n and all(r.at_counts[k].sum() == n for k in range(3))


def test_placed_values():
    state = ops.new_clip_metrics(DEV, THRESHOLDS)
    m = state.margins
    edges = np.arange(-2048, 2049, dtype=np.float32) / np.float32(64.0)                      # every bin edge, +32 included
    below = np.nextafter(m, np.float32(-np.inf))
    placed = np.concatenate([edges, m, below, np.nextafter(m, np.float32(np.inf)), np.float32([40.0, -40.0, 3.0e38, -3.0e38, 0.0, -0.0])])
    z = np.stack([np.zeros_like(placed), placed], axis=1)
    special = np.float32([[0, np.nan], [np.nan, 0], [np.nan, np.nan], [0, np.inf], [0, -np.inf], [np.inf, 0], [-np.inf, 0],
                          [np.inf, np.inf], [-np.inf, -np.inf], [np.inf, -np.inf], [3.0e38, -3.0e38], [-3.0e38, 3.0e38], [1.5, 1.5]])
    z = np.concatenate([z, special, z[:8], z[:8]]).astype(np.float32)
    y = (np.arange(len(z)) % 2).astype(np.int64)
    y[-16:] = [-1, 2, 2 ** 40, -2 ** 40, 3, 2 ** 32, 2 ** 32 + 1, -2] + [0, 1, 0, 1, 1, 1, 0, 0]
    assert _feed(state, z, y) == 1
    r = ops.read_clip_metrics(state)
    want = ref.counters(z, y, m)
    ref.assert_counters(r, want, batches=1)
    assert r.bad_labels == 8 and r.nonfinite == 12 and r.clips_seen == len(z) and r.total == len(z) - 8
    # what the placed values are there for, spelled out (one clip at a time through the same restatement)
    one = lambda zz, yy: ref.counters(np.float32([zz]), [yy], m)                               # noqa: E731
    assert one([0, -32.0], 0)["hist"][0, 0] == 1 and one([0, 32.0], 1)["hist"][1, 4095] == 1
    assert one([0, 1 / 64], 1)["hist"][1, 2049] == 1 and one([0, -1 / 64], 1)["hist"][1, 2047] == 1
    assert one([0, 40.0], 0)["hist"][0, 4095] == 1 and one([0, -40.0], 0)["hist"][0, 0] == 1
    for k in range(3):
        assert one([0, m[k]], 1)["at"][k, 1, 1] == 1 and one([0, below[k]], 1)["at"][k, 1, 0] == 1
    assert one([np.inf, np.inf], 1)["nonfinite"] == 1 and one([np.inf, np.inf], 1)["argmax"][1, 0] == 1
    assert one([0, np.inf], 0)["argmax"][0, 1] == 1 and one([0, np.inf], 0)["hist"].sum() == 0
    # and the device agrees clip by clip on the ones that matter most: a margin on a threshold fires, one step below does not
    for k in range(3):
        for value, fired in ((m[k], 1), (below[k], 0)):
            ops.reset_clip_metrics(state)
            _feed(state, np.float32([[0, value]]), [1])
            got = ops.read_clip_metrics(state)
            assert got.at_counts[k, 1, fired] == 1 and got.at_counts[k].sum() == 1 and got.at(THRESHOLDS[k])["tp"] == fired


def test_batch_size_does_not_matter_and_reset_keeps_the_margins():
    rng = np.random.default_rng(7)
    n = 10000
    z = (rng.standard_normal((n, 2)) * 9.0).astype(np.float32)
    y = (rng.random(n) < 0.1).astype(np.int64)
    y[rng.integers(0, n, 20)] = 5
    z[rng.integers(0, n, 20), 1] = np.inf
    want = ref.counters(z, y, ops.new_clip_metrics(DEV, THRESHOLDS).margins)
    reports = []
    for sizes, calls in (([n], 1), ([16], 625), ([17], 589), ([4096], 3), ([1, 2, 1023, 1024, 1025], None)):
        state = ops.new_clip_metrics(DEV, THRESHOLDS)
        made = _feed(state, z, y, sizes)
        assert calls is None or made == calls
        r = ops.read_clip_metrics(state)
        ref.assert_counters(r, want, batches=made)
        reports.append(r)
    assert all(r == reports[0] for r in reports) and reports[0].auc == reports[3].auc
    # reset: counters to zero, operating points kept; the record counts again from nothing
    ops.reset_clip_metrics(state)
    zero = ops.read_clip_metrics(state)
    assert zero.clips_seen == 0 and zero.batches == 0 and zero.hist.sum() == 0 and zero.at_counts.sum() == 0 and zero.confusion.sum() == 0
    assert np.array_equal(zero.margins, reports[0].margins) and zero.thresholds == THRESHOLDS
    _feed(state, z, y, [4096])
    assert ops.read_clip_metrics(state) == reports[0]
    # no operating points at all, and eight of them
    none = ops.new_clip_metrics(DEV, ())
    _feed(none, z, y)
    r0 = ops.read_clip_metrics(none)
    assert r0.at_counts.shape == (0, 2, 2) and np.array_equal(r0.hist, want["hist"]) and np.array_equal(r0.confusion, want["argmax"])
    eight = tuple(float(p) for p in np.linspace(0.1, 0.9, 8))
    full = ops.new_clip_metrics(DEV, eight)
    _feed(full, z, y, [3000])
    ref.assert_counters(ops.read_clip_metrics(full), ref.counters(z, y, full.margins), batches=4)


def test_update_is_a_pure_launch():
    state = ops.new_clip_metrics(DEV, THRESHOLDS)
    z = torch.randn(4096, 2, device=DEV)
    y = torch.randint(0, 2, (4096, 1), device=DEV)
    ops.clip_metrics_update(z, y, state)                                   # [B, 1] labels are taken as ce_loss takes them
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        before = torch.cuda.memory_allocated()
        for _ in range(3):
            ops.clip_metrics_update(z, y, state)
        ops.reset_clip_metrics(state)
        ops.clip_metrics_update(z[:17], y[:17], state)
        after = torch.cuda.memory_allocated()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert before == after
    r = ops.read_clip_metrics(state)
    assert r.clips_seen == 17 and r.batches == 1
    # the wrapper's checks
    with pytest.raises(RuntimeError):
        ops.clip_metrics_update(z.cpu(), y, state)
    with pytest.raises(TypeError):
        ops.clip_metrics_update(z, y.int(), state)
    with pytest.raises(ValueError):
        ops.clip_metrics_update(z, y[:5], state)
    with pytest.raises(TypeError):
        ops.clip_metrics_update(z, y, ops.new_loss_stats(DEV))
    for bad in ((0.0,), (1.0,), (0.5, float("nan")), (0.5, 0.5), tuple([0.5] * 9)):
        with pytest.raises(ValueError):
            ops.new_clip_metrics(DEV, bad)
    with pytest.raises(RuntimeError):
        ops.new_clip_metrics("cpu")


def _model(seed=1234):
    torch.manual_seed(seed)
    return pkg.SimpleWakewordModel().to(DEV)


def _batch(n, T, seed):
    g = torch.Generator().manual_seed(seed)
    x = (-40.0 + 20.0 * torch.randn(n, 1, 80, T, generator=g)).to(DEV)
    y = torch.randint(0, 2, (n, 1), generator=g).to(DEV)
    return x, y


@pytest.mark.parametrize("T", [32, 9])
def test_validate_keeps_a_report_beside_loss_and_accuracy(T):
    model = _model()
    trainer = pkg.WakewordTrainer(model, DEV, thresholds=THRESHOLDS)
    with pytest.raises(RuntimeError, match="validate"):
        trainer.val_report
    x, y = _batch(37, T, seed=T)
    batches = [(x[i:i + 16], y[i:i + 16]) for i in range(0, 37, 16)]
    _, val_acc = trainer.validate(batches)
    r = trainer.val_report
    assert r is trainer.val_report                                         # read once, kept until the next validate
    # integer for integer: the trainer's percentage is 100 correct / total of THESE integers, and accuracy is correct / total.
    # `accuracy * 100 == val_acc` is the same statement wherever float64 lets it be one: (c / 37) * 100 and 100 c / 37 round apart
    # for c in {9, 17, 18, 19, 34, 36}, whatever computed c.
    correct = int(np.trace(r.confusion))
    assert r.clips_seen == r.total == 37 and r.batches == 3
    assert 100.0 * correct / r.total == val_acc and r.accuracy == correct / 37
    if (correct / 37) * 100 == 100.0 * correct / 37:
        assert r.accuracy * 100 == val_acc
    with torch.no_grad():
        z = torch.cat([model(xb) for xb, _ in batches]).cpu().numpy()
    labels = y[:, 0].cpu().numpy()
    conf = np.zeros((2, 2), np.int64)
    np.add.at(conf, (labels, (z[:, 1] > z[:, 0]).astype(np.int64)), 1)
    assert np.array_equal(r.confusion, conf)
    ref.assert_counters(r, ref.counters(z, labels, trainer.val_metrics.margins), batches=3)
    # one clip 37 times, 12 of them labelled 1: 12 or 25 are correct whatever the model says, and for both the identity holds as written
    y12 = torch.tensor([1] * 12 + [0] * 25, device=DEV).view(37, 1)
    _, acc12 = trainer.validate([(x[:1].repeat(37, 1, 1, 1), y12)])
    assert int(np.trace(trainer.val_report.confusion)) in (12, 25) and trainer.val_report.accuracy * 100 == acc12
    # the next validate starts from zero
    trainer.validate(batches[:1])
    assert trainer.val_report is not r and trainer.val_report.clips_seen == 16


def test_evaluate_report_counts_what_evaluate_predicts():
    model = _model(seed=3)
    x, y = _batch(53, 32, seed=11)
    loader = [(x[i:i + 16].cpu(), y[i:i + 16].cpu()) for i in range(0, 53, 16)]    # a loader on the host, as the reference's
    preds, labels = inference.evaluate(model, loader, DEV)
    r = inference.evaluate_report(model, loader, DEV, thresholds=THRESHOLDS)
    conf = np.zeros((2, 2), np.int64)
    np.add.at(conf, (np.asarray(labels, np.int64), np.asarray(preds, np.int64)), 1)
    assert np.array_equal(r.confusion, conf) and r.batches == 4 and r.total == 53
    assert pkg.evaluate_report is inference.evaluate_report and pkg.ClipReport is type(r)
    r2 = inference.evaluate_report(model, [(x, y[:, 0])])                  # device tensors, [B] labels, the default threshold, no device given
    assert np.array_equal(r2.confusion, conf) and r2.thresholds == (0.8,) and np.array_equal(r2.hist, r.hist)
    assert r2.at(0.8) == r.at(0.8)
    # the PCM form
    clips = torch.from_numpy(pkg.synth.make_clips(0, 24)).to(DEV)
    lab = torch.arange(24, device=DEV) % 2
    logits, pp = inference.evaluate_pcm(model, clips, batch_size=10)
    rp = inference.evaluate_report_pcm(model, clips, batch_size=10, labels=lab, thresholds=THRESHOLDS)
    ref.assert_counters(rp, ref.counters(logits.cpu().numpy(), lab.cpu().numpy(), rp.margins), batches=3)
    with pytest.raises(TypeError):
        inference.evaluate_report_pcm(model, clips)


CKPT_KEYS = sorted(["epoch", "model_state_dict", "optimizer_state_dict", "val_acc", "train_acc", "train_loss", "val_loss"])


def _train_run(tmp_path, capsys, tag, **kw):
    model = _model(seed=21)
    with torch.no_grad():
        model.fc.bias.copy_(torch.tensor([-2.0, 2.0]))                     # the untrained model says "wake word": F1 and AUC are above zero
    path = str(tmp_path / f"{tag}.pth")
    trainer = pkg.WakewordTrainer(model, DEV, checkpoint_path=path, **kw)
    x, y = _batch(48, 8, seed=5)
    train = [(x[i:i + 16], y[i:i + 16]) for i in range(0, 32, 16)]
    val = [(x[32:], y[32:])]
    torch.manual_seed(9)
    best = trainer.train(train, val, epochs=2)
    return trainer, best, capsys.readouterr().out, path, val


def _no_memory_lines(text):
    return [line for line in text.splitlines() if not line.startswith("GPU Memory:")]


def test_train_follows_the_monitor(tmp_path, capsys):
    base, best0, text0, path0, val = _train_run(tmp_path, capsys, "plain")
    with pytest.raises(ValueError, match="monitor"):
        pkg.WakewordTrainer(_model(), DEV, monitor="val_loss")
    for monitor in ("val_acc", "val_f1", "val_auc"):
        t, best, text, path, _ = _train_run(tmp_path, capsys, monitor, monitor=monitor)
        assert len(t.monitor_history) == 2 and t.monitor == monitor
        assert sorted(torch.load(path, weights_only=True)) == CKPT_KEYS
        # the same seeds give the same two epochs whatever is monitored
        assert t.val_accuracies == base.val_accuracies and t.val_losses == base.val_losses and t.train_losses == base.train_losses
        # the second epoch's monitored value is the one val_report still holds
        t.validate(val)
        rep = t.val_report
        want = {"val_acc": t.val_accuracies[1], "val_f1": 100.0 * rep.f1, "val_auc": 100.0 * rep.auc}[monitor]
        assert t.monitor_history[1] == want
        top, best_epoch = 0.0, None                                        # the reference's rule: a strict improvement on 0.0
        for i, v in enumerate(t.monitor_history):
            if v > top:
                top, best_epoch = v, i
        assert best_epoch is not None and t.best_monitor == top
        assert best == t.best_val_acc == t.val_accuracies[best_epoch]
        assert torch.load(path, weights_only=True)["val_acc"] == t.val_accuracies[best_epoch]
        if monitor == "val_acc":
            assert t.monitor_history == t.val_accuracies and best == best0
            assert _no_memory_lines(text) == _no_memory_lines(text0)       # the prints of a trainer built without the keyword
            assert t.train_accuracies == base.train_accuracies
        else:
            assert f"Val {'F1' if monitor == 'val_f1' else 'AUC'}: {t.monitor_history[0]:.2f}%" in text
