"""Mixup and the soft-target cross-entropy on the GPU (ww_ce_loss_soft_f32 in csrc/ww_optim.hip, ww_mixup_f32
in csrc/ww_mixup.hip): the two kernels, WakewordTrainer's fused step on class probabilities, and the loaders under set_mixup.

Tolerances.  The soft loss follows tests/test_gpu_loss.py: the reference for a float32 quantity is torch's own float32 result on the same
device and inputs (F.cross_entropy with probability targets); its error against the float64 restatement of tests/mixup_ref.py is
measured here and must stay under a fixed cap; ours may be at most twice that plus 2^-24 (trainer_ref.allowed).  A mixed element is
within 1.6e-5 of its float64 value: at most two float32 roundings of magnitudes below 128, each at most 2^-24 * 128.  Everything else --
one-hot targets against the integer-label kernel, copied rows, targets, repeats, loaders against a hand-written loop -- is bit for bit.

Out-of-range partners used on the device are -1 and B only, and the mel batch then sits between two spare rows of its own buffer."""
import os
import random

import numpy as np
import pytest
import torch
import torch.nn as nn

import loss_ref
import mixup_ref as ref
import trainer_ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import ops, synth
from wakeword_jupyterlab_amd.config import AudioConfig, MixupConfig
from wakeword_jupyterlab_amd.ledger import ClipLedger

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = ref.U
GUARD = -77.25


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rule(name, ours, torchs, cap):
    print(f"{name}: ours {ours / U:.3f} u, torch {torchs / U:.3f} u (u = 2^-24)")
    assert torchs <= cap, f"{name}: the REFERENCE's own error {torchs / U:.3f} u exceeds its cap {cap / U:.1f} u (torch on this device, not the kernel)"
    assert ours <= trainer_ref.allowed(torchs), f"{name}: {ours / U:.3f} u > 2 x {torchs / U:.3f} u + 1 u"


def _same_float(a, b):
    return a == b or (a != a and b != b)


# ======================================================================================================================================
# the soft loss
# ======================================================================================================================================
@pytest.mark.parametrize("n", loss_ref.SIZES)
def test_one_hot_targets_have_the_bits_of_the_integer_label_kernel(n):
    z, y = trainer_ref.ce_inputs(n, seed=n)
    zt, yt, tt = _dev(z), _dev(y), _dev(ref.one_hot(y))
    for hard_kw, soft_kw in (({}, {}), ({}, dict(weight=(1.0, 1.0), label_smoothing=0.0)), (dict(reduction="sum"), dict(reduction="sum")),
                             (dict(reduction="sum"), dict(reduction="sum", weight=(1.0, 1.0)))):
        s_hard, s_soft = ops.new_loss_stats(DEV), ops.new_loss_stats(DEV)
        loss, d = ops.ce_loss(zt, yt, s_hard, **hard_kw)
        loss2, d2 = ops.soft_ce_loss(zt, tt, s_soft, **soft_kw)
        assert torch.equal(loss, loss2) and torch.equal(d, d2) and torch.equal(s_hard, s_soft), (hard_kw, soft_kw)
        assert ops.read_loss_stats(s_soft)["batches"] == 1


def _soft_case(case, n, z, t):
    tag, opts = case["tag"], case["opts"]
    want = ref.restate(case, z, t)
    zt, tt = _dev(z), _dev(t)
    stats = ops.new_loss_stats(DEV)
    loss, d = ops.soft_ce_loss(zt, tt, stats, **opts)
    lt, dt = ref.torch_reference(case, z, t, DEV)
    _rule(f"{tag} loss", loss_ref.loss_error(float(loss), want["loss"]), loss_ref.loss_error(lt, want["loss"]), ref.CAP_SOFT_LOSS)
    _rule(f"{tag} dlogits", loss_ref.dlogits_error(_np(d), want), loss_ref.dlogits_error(dt, want), ref.CAP_SOFT_DLOGITS)
    s = ops.read_loss_stats(stats)
    assert (s["correct"], s["total"], s["batches"], s["bad_labels"], s["nonfinite"]) == (want["correct"], n, 1, 0, 0), tag
    assert _same_float(s["loss_sum"], float(loss)), tag
    # a second run is bit-equal
    loss2, d2 = ops.soft_ce_loss(zt, tt, **opts)
    assert torch.equal(d, d2) and torch.equal(loss, loss2), tag
    # logits, targets and gradient 4 bytes off the 16-byte grid: the same bits, guard words intact
    zb, tb = torch.zeros(2 * n + 1, device=DEV), torch.zeros(2 * n + 1, device=DEV)
    zb[1:], tb[1:] = zt.reshape(-1), tt.reshape(-1)
    loss3 = torch.empty((), device=DEV)
    d3 = torch.full((2 * n + 2,), GUARD, device=DEV)
    ops.soft_ce_loss_into(zb[1:].view(n, 2), tb[1:].view(n, 2), d3[1:2 * n + 1].view(n, 2), loss3, None, **opts)
    assert torch.equal(d3[1:2 * n + 1].view(n, 2), d) and torch.equal(loss3, loss) and d3[0] == GUARD and d3[-1] == GUARD, tag
    # the validation form writes no gradient: logits, then a canary where one would go
    both = torch.full((4 * n,), GUARD, device=DEV)
    both[:2 * n] = zt.reshape(-1)
    loss4 = torch.empty((), device=DEV)
    ops.soft_ce_loss_into(both[:2 * n].view(n, 2), tt, None, loss4, None, **opts)
    assert torch.all(both[2 * n:] == GUARD) and torch.equal(loss4, loss), tag


@pytest.mark.parametrize("n", loss_ref.SIZES)
def test_soft_loss_against_float64(n):
    z, t = ref.soft_inputs(n)
    for case in ref.soft_cases(n):
        _soft_case(case, n, z, t)


def test_bad_target_rows_are_left_out_and_counted():
    n = 130
    z, t = ref.soft_inputs(n)
    t = t.copy()
    t[0], t[64], t[129] = (np.nan, 0.5), (np.inf, 0.0), (-0.25, 1.25)
    keep = np.ones(n, bool)
    keep[[0, 64, 129]] = False
    zt, tt = _dev(z), _dev(t)
    for case in ref.soft_cases(n):
        opts = case["opts"]
        want = ref.restate(case, z[keep], t[keep])                                  # the restatement over the rest
        assert ref.restate(case, z, t)["loss"] == pytest.approx(want["loss"], rel=1e-13) and want["counted"] == 127
        stats = ops.new_loss_stats(DEV)
        d = torch.full((n, 2), GUARD, device=DEV)
        loss = torch.zeros((), device=DEV)
        ops.soft_ce_loss_into(zt, tt, d, loss, stats, **opts)
        assert torch.all(d[_dev(~keep)] == 0.0), case["tag"]                         # exactly zero, not GUARD and not NaN
        lt, dt = ref.torch_reference(case, z[keep], t[keep], DEV)
        _rule(f"{case['tag']} bad rows: loss", loss_ref.loss_error(float(loss), want["loss"]), loss_ref.loss_error(lt, want["loss"]), ref.CAP_SOFT_LOSS)
        _rule(f"{case['tag']} bad rows: dlogits", loss_ref.dlogits_error(_np(d)[keep], want), loss_ref.dlogits_error(dt, want), ref.CAP_SOFT_DLOGITS)
        s = ops.read_loss_stats(stats)
        assert (s["bad_labels"], s["total"], s["correct"], s["nonfinite"]) == (3, n, want["correct"], 0), case["tag"]
    # nothing counted: a NaN mean, a zero sum, and a gradient of zeros either way
    for bad in (np.nan, -1.0, np.inf):
        none = torch.full((n, 2), bad, device=DEV)
        for kw in (dict(), dict(weight=(0.25, 4.0), label_smoothing=0.125)):
            stats = ops.new_loss_stats(DEV)
            d = torch.full((n, 2), GUARD, device=DEV)
            loss = torch.zeros((), device=DEV)
            ops.soft_ce_loss_into(zt, none, d, loss, stats, **kw)
            assert torch.isnan(loss) and not d.any()
            s = ops.read_loss_stats(stats)
            assert (s["correct"], s["total"], s["bad_labels"]) == (0, n, n) and s["loss_sum"] != s["loss_sum"]
            loss_sum, d_sum = ops.soft_ce_loss(zt, none, reduction="sum", **kw)
            assert float(loss_sum) == 0.0 and not d_sum.any()


def test_nonfinite_logits_are_counted_as_in_the_integer_label_kernel():
    n = 130
    z, y = trainer_ref.ce_inputs(n, seed=9)
    z = z.copy()
    z[1], z[65], z[129] = (np.nan, 0.0), (0.0, np.inf), (-np.inf, 1.0)
    s_hard, s_soft = ops.new_loss_stats(DEV), ops.new_loss_stats(DEV)
    ops.ce_loss(_dev(z), _dev(y), s_hard)
    ops.soft_ce_loss(_dev(z), _dev(ref.one_hot(y)), s_soft)
    hard, soft = ops.read_loss_stats(s_hard), ops.read_loss_stats(s_soft)
    assert soft["nonfinite"] == hard["nonfinite"] == 3 and soft["correct"] == hard["correct"] and soft["bad_labels"] == 0


def test_ops_refuse_bad_arguments_before_any_launch():
    z, t = torch.zeros(4, 2, device=DEV), torch.full((4, 2), 0.5, device=DEV)
    d = torch.full((4, 2), GUARD, device=DEV)
    for kw in (dict(weight=(1.0,)), dict(weight=(1.0, -1.0)), dict(label_smoothing=1.5), dict(reduction="max")):
        with pytest.raises(ValueError):
            ops.soft_ce_loss_into(z, t, d, None, None, **kw)
    for kw in (dict(reduction="none"), dict(focal_gamma=2.0)):
        with pytest.raises(NotImplementedError):
            ops.soft_ce_loss(z, t, **kw)
    for bad in (torch.zeros(4, dtype=torch.int64, device=DEV), t.double(), t.cpu()):
        with pytest.raises((TypeError, RuntimeError)):
            ops.soft_ce_loss(z, bad)
    for bad in (t[:3], torch.zeros(4, 3, device=DEV), torch.zeros(2, 4, device=DEV).t()):
        with pytest.raises(ValueError):
            ops.soft_ce_loss(z, bad)
    with pytest.raises(TypeError):
        ops.ce_loss(z, t)                                                           # the integer-label entry is as it was
    assert torch.all(d == GUARD)
    loss, _ = ops.soft_ce_loss(z, t)
    assert abs(float(loss) - np.log(2.0)) <= U


# ======================================================================================================================================
# the mixup kernel
# ======================================================================================================================================
def _guarded(n_floats, offset=0, pad=64):
    """A float32 buffer of `n_floats` between two guard bands of `pad` floats, `offset` floats off the 16-byte grid."""
    raw = torch.full((n_floats + 2 * pad + offset,), GUARD, device=DEV)
    assert raw.data_ptr() % 16 == 0
    return raw, raw[pad + offset:pad + offset + n_floats]


def _guards_intact(raw, n_floats, offset=0, pad=64):
    return bool(torch.all(raw[:pad + offset] == GUARD)) and bool(torch.all(raw[pad + offset + n_floats:] == GUARD))


def _mix_call(mel_rows, labels, partner, lam, offset=0):
    """ops.mixup_into on a mel batch that sits between two spare rows of its buffer, into guarded out and targets."""
    B, rest = mel_rows.shape[0], mel_rows.shape[1:]
    row = int(np.prod(rest))
    src = torch.zeros((B + 2) * row + offset, device=DEV)
    mel = src[offset + row:offset + (B + 1) * row].view(B, *rest)
    mel.copy_(mel_rows)
    raw_o, out = _guarded(B * row, offset)
    raw_t, tg = _guarded(2 * B, offset)
    ops.mixup_into(mel, _dev(labels), _dev(partner), _dev(lam), out.view(B, *rest), tg.view(B, 2))
    assert _guards_intact(raw_o, B * row, offset) and _guards_intact(raw_t, 2 * B, offset), "a guard band was written"
    assert (mel.data_ptr() % 16 == 0) == (offset == 0) and (out.data_ptr() % 16 == 0) == (offset == 0)
    return out.view(B, *rest).clone(), tg.view(B, 2).clone()


@pytest.mark.parametrize("T", ref.MIX_T)
@pytest.mark.parametrize("B", ref.MIX_B)
def test_mixup_kernel(B, T):
    mel, labels, partner, lam = ref.mix_inputs(B, T)
    want, want_t, mixed = ref.mixup(mel, labels, partner, lam)
    assert B == 1 or mixed.any()
    melt = _dev(mel)
    out, tg = _mix_call(melt, labels, partner, lam)
    got = _np(out)
    assert np.array_equal(got[~mixed].view(np.int32), mel[~mixed].view(np.int32))    # copied rows: the input's bits
    err = float(np.abs(got[mixed].astype(np.float64) - want[mixed]).max()) if mixed.any() else 0.0
    print(f"B={B} T={T}: mixed rows {int(mixed.sum())}, max |out - float64| = {err:.3e} (bound {ref.MIX_TOL:.1e})")
    assert err <= ref.MIX_TOL
    assert np.array_equal(_np(tg), want_t, equal_nan=True)                          # the targets are exact
    if B >= 5:
        assert np.isnan(want_t[[0, 1, 2]]).all() and want_t[3].tolist() == [0.875, 0.125] and want_t[4].tolist() == [0.0, 1.0]
    # two runs give identical bits; so does the public form that allocates; so does the scalar path of a 4-byte-offset view
    out2, tg2 = _mix_call(melt, labels, partner, lam)
    out3, tg3 = ops.mixup(melt.view(B, 1, 80, T), _dev(labels)[:, None], _dev(partner), _dev(lam))
    out4, tg4 = _mix_call(melt, labels, partner, lam, offset=1)
    for o, t in ((out2, tg2), (out3.view(B, 80, T), tg3), (out4, tg4)):
        assert torch.equal(o.view(torch.int32), out.view(torch.int32)) and torch.equal(t.view(torch.int32), tg.view(torch.int32))
    # an unmixed row does not read its partner: the partner row is NaN, the row comes out as it went in
    if B >= 2:
        poisoned = mel.copy()
        poisoned[1] = np.nan
        lam1, partner1 = lam.copy(), partner.copy()
        lam1[0], partner1[0] = 1.0, 1
        out5, tg5 = _mix_call(_dev(poisoned), labels, partner1, lam1)
        assert np.array_equal(_np(out5)[0].view(np.int32), mel[0].view(np.int32))
        assert _np(tg5)[0].tolist() == ([1.0, 0.0] if labels[0] == 0 else [0.0, 1.0])
    # a partner outside [0, B): the row as it went in, a NaN target -- whatever lambda says
    for bad in (-1, B):
        for row, lam_row in ((0, 0.75), (B - 1, 1.0)):
            partner2, lam2 = partner.copy(), lam.copy()
            partner2[row], lam2[row] = bad, lam_row
            want2, want_t2, mixed2 = ref.mixup(mel, labels, partner2, lam2)
            out6, tg6 = _mix_call(melt, labels, partner2, lam2)
            assert not mixed2[row] and np.isnan(want_t2[row]).all()
            assert np.array_equal(_np(out6)[row].view(np.int32), mel[row].view(np.int32))
            assert np.array_equal(_np(tg6), want_t2, equal_nan=True)


def test_mixup_ops_refuse_bad_arguments_before_any_launch():
    mel = torch.zeros(4, 80, 8, device=DEV)
    y, p, lam = torch.zeros(4, dtype=torch.int64, device=DEV), torch.arange(4, dtype=torch.int32, device=DEV), torch.ones(4, device=DEV)
    out, tg = torch.full_like(mel, GUARD), torch.full((4, 2), GUARD, device=DEV)
    for args in ((mel, y.int(), p, lam), (mel, y, p.long(), lam), (mel, y, p, lam.double()), (mel, y.cpu(), p, lam)):
        with pytest.raises(TypeError):
            ops.mixup_into(*args, out, tg)
    for args in ((mel, y[:3], p, lam), (mel, y, p[:3], lam), (mel, y, p, lam[:3]), (mel.double(), y, p, lam), (mel[:, :, ::2], y, p, lam),
                 (torch.zeros(4, 79, 8, device=DEV), y, p, lam)):
        with pytest.raises(ValueError):
            ops.mixup_into(*args, out, tg)
    with pytest.raises(NotImplementedError):
        ops.mixup(torch.zeros(2, 80, 64, device=DEV), y[:2], p[:2], lam[:2])
    for o, t in ((out[:3], tg), (out, tg[:3]), (out.double(), tg), (out, tg.double())):
        with pytest.raises(ValueError):
            ops.mixup_into(mel, y, p, lam, o, t)
    with pytest.raises(pkg._native.NativeError, match="overlap"):
        ops.mixup_into(mel, y, p, lam, mel, tg)                                     # the kernel works out of place
    assert torch.all(out == GUARD) and torch.all(tg == GUARD)


# ======================================================================================================================================
# trainer
# ======================================================================================================================================
B, T = 16, 8
MODELS = {"simple": pkg.SimpleWakewordModel, "full": pkg.WakewordModel}
W = (0.25, 4.0)


def _batch(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = (-40.0 + 20.0 * torch.randn(n, 1, 80, T, generator=g)).to(DEV)
    y = torch.randint(0, 2, (n, 1), generator=g).to(DEV)
    return x, y


def _model(name, seed=1234):
    torch.manual_seed(seed)
    return MODELS[name]().to(DEV)


def _soft_targets(n):
    return _dev(ref.soft_inputs(n, seed=77)[1])


@pytest.mark.parametrize("name", ["simple", "full"])
def test_trainer_steps_on_one_hot_float_targets_as_on_integer_labels(name):
    model, twin = _model(name), _model(name)
    soft, hard = pkg.WakewordTrainer(model, DEV), pkg.WakewordTrainer(twin, DEV)
    model.train(); twin.train()
    for k in range(3):
        x, y = _batch(B, seed=10 + k)
        t = _dev(ref.one_hot(_np(y)[:, 0]))
        torch.manual_seed(70 + k)
        soft.step(x, t)                  # without the feature this very first call raises: _target refused floating-point targets
        torch.manual_seed(70 + k)
        hard.step(x, y)
        assert torch.equal(soft.last_loss, hard.last_loss), k
    for (k, p), q in zip(model.named_parameters(), twin.parameters()):
        assert torch.equal(p, q), k
    assert torch.equal(soft.train_stats, hard.train_stats)


@pytest.mark.parametrize("name", ["simple", "full"])
def test_trainer_computes_the_soft_criterion_it_holds(name):
    crit = nn.CrossEntropyLoss(weight=torch.tensor(W, device=DEV), label_smoothing=0.125)
    opts = dict(weight=W, label_smoothing=0.125)
    model, twin = _model(name), _model(name)
    trainer = pkg.WakewordTrainer(model, DEV, criterion=crit)
    model.train(); twin.train()
    x, _ = _batch(B, seed=3)
    t = _soft_targets(B)
    torch.manual_seed(77)
    trainer.step(x, t)
    # ---- d loss / d logits: torch's autograd of the criterion on the step's own logits is the reference ----
    logits = trainer.last_logits[:B].clone()
    zr = logits.clone().requires_grad_()
    lt = crit(zr, t)
    lt.backward()
    want = ref.soft_loss(_np(logits), _np(t), W, 0.125, "mean")
    _rule(f"{name} dlogits", loss_ref.dlogits_error(_np(trainer._dlogits[:B]), want), loss_ref.dlogits_error(_np(zr.grad), want), ref.CAP_SOFT_DLOGITS)
    _rule(f"{name} loss", loss_ref.loss_error(float(trainer.last_loss), want["loss"]), loss_ref.loss_error(float(lt.detach()), want["loss"]), ref.CAP_SOFT_LOSS)
    # ---- the parameter gradients: autograd through the same kernels, fed this loss's d loss / d logits (section 3h's identity) ----
    torch.manual_seed(77)
    out = twin(x)
    assert torch.equal(out.detach(), logits)
    out.backward(gradient=ops.soft_ce_loss(out.detach(), t, **opts)[1])
    tnamed = dict(twin.named_parameters())
    for k, p in model.named_parameters():
        assert torch.equal(p.grad, tnamed[k].grad), k
    # ---- a step has no hidden wait and allocates nothing ----
    trainer.step(x, t)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        trainer.step(x, t)
        before = torch.cuda.memory_allocated()
        trainer.step(x, t)
        after = torch.cuda.memory_allocated()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert before == after


def test_trainer_refusals_with_soft_targets_come_before_any_launch():
    x, y = _batch(B, seed=5)
    t = _soft_targets(B)
    for crit, exc in ((pkg.FocalLoss(2.0), NotImplementedError), (nn.CrossEntropyLoss(ignore_index=1), ValueError)):
        model = _model("simple")
        trainer = pkg.WakewordTrainer(model, DEV, criterion=crit)
        model.train()
        before = [p.detach().clone() for p in model.parameters()]
        with pytest.raises(exc):
            trainer.step(x, t)
        assert ops.read_loss_stats(trainer.train_stats)["batches"] == 0 and trainer._logits is None      # nothing ran, nothing was allocated
        assert all(torch.equal(p, q) for p, q in zip(model.parameters(), before))
        trainer.step(x, y)                                                          # integer labels still go through
    trainer = pkg.WakewordTrainer(_model("simple"), DEV)
    with pytest.raises(TypeError, match="integer"):
        trainer.validate([(x, t)])
    trainer.model.train()
    for bad in (t[:, :1], t[:8], t.double()):
        with pytest.raises((ValueError, TypeError)):
            trainer.step(x, bad)
    with pytest.raises(TypeError, match="labels"):                                  # a ledger needs the rows' integer labels
        led = pkg.WakewordTrainer(_model("simple"), DEV, ledger=ClipLedger(4, DEV))
        led.model.train()
        led.step(x, t, entries=np.zeros(B, np.int64))
    bad = t.clone()
    bad[3] = float("nan")                                                           # what ops.mixup writes for a label outside {0, 1}
    with pytest.raises(ValueError, match="labels"):
        trainer.train_epoch([(x, bad)])


# ======================================================================================================================================
# loaders
# ======================================================================================================================================
N_FILES, LB = 24, 8
BAD_FILE = 13
Quarter = type("AudioConfigQuarter", (AudioConfig,), {"DURATION": 0.25})


class _Always(MixupConfig):
    PROB = 1.0


class _Never(MixupConfig):
    PROB = 0.0


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("mixup")
    clips = synth.make_clips(0, N_FILES, n=4000)
    paths = []
    for i in range(N_FILES):
        paths.append(os.path.join(d, f"clip_{i:02d}.wav"))
        if i == BAD_FILE:
            with open(paths[-1], "wb") as f:
                f.write(b"this is not a RIFF file" * 8)
        else:
            synth.write_wav16(paths[-1], clips[i])
    return paths


def _dataset(files, config):
    proc = pkg.AudioProcessor(Quarter, device=DEV)
    proc.set_mixup(config)
    return pkg.WakewordDataset(files[:N_FILES // 2], files[N_FILES // 2:], proc, augment=True, verbose=False)


def _run(loader, seed=3):
    """One epoch with python's generator re-seeded before every batch, so that a batch's draws do not depend on how many the batches
    before it made: (data, target, last_entries, last_labels) per batch."""
    torch.manual_seed(seed)
    out, it, k = [], iter(loader), 0
    while True:
        random.seed(1000 * seed + k)
        try:
            d, t = next(it)
        except StopIteration:
            break
        out.append((d.clone(), t.clone(), loader.last_entries.copy(), loader.last_labels.clone()))
        k += 1
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def control(files):
    """The loaders as they are without the feature: a processor that never heard of mixup."""
    out = {}
    for kind in ("files", "bank"):
        proc = pkg.AudioProcessor(Quarter, device=DEV)
        ds = pkg.WakewordDataset(files[:N_FILES // 2], files[N_FILES // 2:], proc, augment=True, verbose=False)
        out[kind] = _run(ds.loader(LB) if kind == "files" else ds.cache().loader(LB, augment=True))
    return out


def _loader(ds, kind):
    return ds.loader(LB) if kind == "files" else ds.cache().loader(LB, augment=True)


@pytest.mark.parametrize("kind", ("files", "bank"))
def test_loaders_mix_last_and_equal_a_hand_written_mixup(files, control, kind, monkeypatch):
    ds = _dataset(files, MixupConfig)
    proc = ds.processor
    loader = _loader(ds, kind)
    states, plain = [], []
    plan, batch = proc.mixup_plan, proc.mixup_batch
    monkeypatch.setattr(proc, "mixup_plan", lambda *a, **kw: (states.append(random.getstate()), plan(*a, **kw))[1])
    monkeypatch.setattr(proc, "mixup_batch", lambda data, *a, **kw: (plain.append(data.clone()), batch(data, *a, **kw))[1])
    got = _run(loader)
    again = _run(loader)
    assert [g[0].shape[0] for g in got] == [LB] * 3 and len(states) == 6
    mixed_rows = 0
    for k, (data, target, entries, labels) in enumerate(got):
        assert torch.equal(data, again[k][0]) and torch.equal(target.view(torch.int32), again[k][1].view(torch.int32))       # the same seeds, the same bits
        assert target.dtype == torch.float32 and target.shape == (LB, 2) and labels.dtype == torch.int64
        want_labels = np.asarray(ds.labels[k * LB:(k + 1) * LB])
        assert np.array_equal(_np(labels), want_labels)                                                 # the rows' own labels
        bad = np.arange(k * LB, (k + 1) * LB) == BAD_FILE
        # the un-mixed batch is what the loader yields without the feature, after SpecAugment and after bad rows are zeroed
        assert torch.equal(plain[k], control[kind][k][0]) and (not bad.any() or not plain[k][int(np.argmax(bad))].any())
        # the plan, drawn again from the state the loader drew it from, applied by hand
        random.setstate(states[k])
        partner, lam = plan(LB, bad=bad)
        want_data, want_target = ops.mixup(plain[k], labels, _dev(partner), _dev(lam))
        assert torch.equal(data, want_data) and torch.equal(target.view(torch.int32), want_target.view(torch.int32))
        assert (lam[bad] == 1.0).all() and (lam[bad[partner]] == 1.0).all()
        # the ledger's view: -1 exactly on mixed rows and on the unreadable file
        own = np.where(bad, -1, np.arange(k * LB, (k + 1) * LB))
        assert np.array_equal(entries, np.where(lam != 1.0, -1, own)) and entries.dtype == np.int64
        assert np.array_equal(control[kind][k][2], own)
        mixed_rows += int((lam != 1.0).sum())
    assert 0 < mixed_rows < 3 * LB


@pytest.mark.parametrize("kind", ("files", "bank"))
def test_loaders_with_mixup_off_or_at_prob_0_are_what_they_were(files, control, kind):
    for config in (None, _Never):
        ds = _dataset(files, config)
        got = _run(_loader(ds, kind))
        assert len(got) == len(control[kind]) == 3
        for (data, target, entries, labels), (cdata, ctarget, centries, clabels) in zip(got, control[kind]):
            assert torch.equal(data, cdata) and np.array_equal(entries, centries) and torch.equal(labels, clabels)
            if config is None:
                assert target.dtype == torch.int64 and torch.equal(target, ctarget)
            else:
                assert torch.equal(target, _dev(ref.one_hot(_np(ctarget)[:, 0])))
    # mixup belongs to augmentation: a validation loader draws nothing and yields integer labels
    proc = pkg.AudioProcessor(Quarter, device=DEV)
    proc.set_mixup(_Always)
    val = pkg.WakewordDataset(files[:4], files[20:], proc, augment=False, verbose=False)
    random.seed(1)
    state = random.getstate()
    for loader in (val.loader(LB), val.cache().loader(LB)):
        for data, target in loader:
            assert target.dtype == torch.int64
        assert random.getstate() == state


def test_file_loader_and_bank_loader_agree_with_mixup_on(files):
    ds = _dataset(files, _Always)
    a, b = _run(ds.loader(LB), seed=5), _run(ds.cache().loader(LB, augment=True), seed=5)
    assert len(a) == len(b) == 3
    for x, y in zip(a, b):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1].view(torch.int32), y[1].view(torch.int32)) and np.array_equal(x[2], y[2])
        assert torch.equal(x[3], y[3])
    assert sum(int((x[2] == -1).sum()) for x in a) >= 3 * LB - 6                     # PROB = 1: all mixed but rounding to lam = 1 and bad rows


class _Recording:
    """A loader that keeps every batch's last_entries, for the ledger's arithmetic."""

    def __init__(self, loader):
        self.loader, self.seen = loader, []

    def __iter__(self):
        for batch in self.loader:
            self.last_entries, self.last_labels = self.loader.last_entries, self.loader.last_labels
            self.seen.append(self.last_entries.copy())
            yield batch


def test_ledger_sees_only_unmixed_rows(files):
    ds = _dataset(files, MixupConfig)
    bank = ds.cache()
    ledger = ClipLedger.for_bank(bank)
    torch.manual_seed(0)
    model = pkg.SimpleWakewordModel(audio_config=Quarter).to(DEV)
    trainer = pkg.WakewordTrainer(model, DEV, ledger=ledger)
    loader = _Recording(bank.loader(LB, augment=True))
    random.seed(4)
    loss, acc = trainer.train_epoch(loader)
    assert np.isfinite(loss)
    rep = ledger.read()
    entries = np.concatenate(loader.seen)
    want = np.bincount(entries[entries >= 0], minlength=bank.n_entries)
    assert np.array_equal(rep.seen, want) and rep.header["skipped"] == int((entries < 0).sum()) and rep.header["rows"] == N_FILES
    assert 0 < want.sum() < N_FILES - 1 and rep.header["bad_labels"] == 0 and want[BAD_FILE] == 0

