"""The loss for imbalanced data on the GPU (ww_ce_loss_ex_f32 in csrc/ww_optim.hip): class weights, label
smoothing, ignore_index, a sum reduction and the focal loss, in the kernel and in WakewordTrainer's fused step.

Tolerances (tests/loss_ref.py, the rule of tests/trainer_ref.py): the reference for a float32 quantity is torch's own float32 result on
the same device and inputs -- F.cross_entropy with the same options, or the expression of FocalLoss.forward; its error against the float64
restatement is measured here and must stay under a fixed cap; ours may be at most twice that plus 2^-24."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import loss_ref as ref
import trainer_ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = ref.U
GUARD = -77.25


def _np(t):
    return t.detach().cpu().numpy()


def _rule(name, ours, torchs, cap):
    print(f"{name}: ours {ours / U:.3f} u, torch {torchs / U:.3f} u (u = 2^-24)")
    assert torchs <= cap, f"{name}: the REFERENCE's own error {torchs / U:.3f} u exceeds its cap {cap / U:.1f} u (torch on this device, not the kernel)"
    assert ours <= trainer_ref.allowed(torchs), f"{name}: {ours / U:.3f} u > 2 x {torchs / U:.3f} u + 1 u"


def _caps(opts):
    return (ref.CAP_FOCAL_LOSS, ref.CAP_FOCAL_DLOGITS) if opts.get("focal_gamma") is not None else (ref.CAP_CE_LOSS, ref.CAP_CE_DLOGITS)


def _same_float(a, b):
    return a == b or (a != a and b != b)


# ======================================================================================================================================
# kernel
# ======================================================================================================================================
def _kernel_case(case, n):
    tag, opts = case["tag"], case["opts"]
    z, y = ref.case_inputs(n, case["labels"], case["extra"])
    want = ref.restate(case, z, y)
    zt, yt = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
    stats = ops.new_loss_stats(DEV)
    loss, d = ops.ce_loss(zt, yt, stats, **opts)
    lt, dt = ref.torch_reference(case, z, y, DEV, pkg.FocalLoss)
    if want["denom"] > 0.0:
        cap_loss, cap_d = _caps(opts)
        _rule(f"{tag} loss", ref.loss_error(float(loss), want["loss"]), ref.loss_error(lt, want["loss"]), cap_loss)
        _rule(f"{tag} dlogits", ref.dlogits_error(_np(d), want), ref.dlogits_error(dt, want), cap_d)
    else:                                                           # nothing counted: NaN as torch gives, and a gradient of zeros
        assert float(loss) != float(loss) and lt != lt, tag
        assert not d.any(), tag
    counted = (y != opts.get("ignore_index", -100)) & ((y == 0) | (y == 1))
    assert torch.all(d[torch.from_numpy(~counted).to(DEV)] == 0.0), tag       # exact zeros where a clip is ignored or its label is bad
    s = ops.read_loss_stats(stats)
    assert (s["correct"], s["total"], s["batches"], s["bad_labels"], s["nonfinite"]) == (want["correct"], n, 1, want["bad"], 0), tag
    assert _same_float(s["loss_sum"], float(loss)), tag
    # a second run is bit-equal
    loss2, d2 = ops.ce_loss(zt, yt, **opts)
    assert torch.equal(d, d2) and _same_float(float(loss), float(loss2)), tag
    # logits and gradient 4 bytes off the 16-byte grid: the same bits, guard words intact
    buf = torch.zeros(2 * n + 1, device=DEV)
    buf[1:] = zt.reshape(-1)
    loss3 = torch.empty((), device=DEV)
    d3 = torch.full((2 * n + 2,), GUARD, device=DEV)
    ops.ce_loss_into(buf[1:].view(n, 2), yt, d3[1:2 * n + 1].view(n, 2), loss3, None, **opts)
    assert torch.equal(d3[1:2 * n + 1].view(n, 2), d) and _same_float(float(loss3), float(loss)) and d3[0] == GUARD and d3[-1] == GUARD, tag
    # the validation form writes no gradient: logits, then a canary where one would go
    both = torch.full((4 * n,), GUARD, device=DEV)
    both[:2 * n] = zt.reshape(-1)
    loss4 = torch.empty((), device=DEV)
    ops.ce_loss_into(both[:2 * n].view(n, 2), yt, None, loss4, None, **opts)
    assert torch.all(both[2 * n:] == GUARD) and _same_float(float(loss4), float(loss)), tag


@pytest.mark.parametrize("n", ref.SIZES)
def test_loss_kernel_against_float64(n):
    for case in ref.kernel_cases(n):
        _kernel_case(case, n)


@pytest.mark.parametrize("n", ref.SIZES)
def test_everything_ignored_is_a_nan_loss_and_a_zero_gradient(n):
    z, _ = trainer_ref.ce_inputs(n, seed=n)
    zt = torch.from_numpy(z).to(DEV)
    yt = torch.full((n,), -100, dtype=torch.int64, device=DEV)
    for opts in (dict(weight=(0.25, 4.0), label_smoothing=0.125), dict(focal_gamma=2.0), dict(ignore_index=-100, weight=(1.0, 1.0))):
        stats = ops.new_loss_stats(DEV)
        d = torch.full((n, 2), GUARD, device=DEV)
        loss = torch.zeros((), device=DEV)
        ops.ce_loss_into(zt, yt, d, loss, stats, **opts)
        assert torch.isnan(loss) and not d.any()
        s = ops.read_loss_stats(stats)
        assert (s["correct"], s["total"], s["bad_labels"]) == (0, n, 0) and s["loss_sum"] != s["loss_sum"]
        loss_sum, _ = ops.ce_loss(zt, yt, reduction="sum", **opts)                # a sum over nothing is 0
        assert float(loss_sum) == 0.0


@pytest.mark.parametrize("n", ref.SIZES)
def test_default_options_are_the_plain_call_and_unit_options_keep_its_bits(n):
    z, y = trainer_ref.ce_inputs(n, seed=n)
    zt, yt = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
    loss, d = ops.ce_loss(zt, yt)
    loss1, d1 = ops.ce_loss(zt, yt, weight=None, label_smoothing=0.0, ignore_index=-100, reduction="mean", focal_gamma=None)
    assert torch.equal(loss, loss1) and torch.equal(d, d1)
    # the extended kernel with unit weights, no smoothing and nothing ignored: the same arithmetic, the same bits
    loss2, d2 = ops.ce_loss(zt, yt, ignore_index=-1)
    assert torch.equal(loss, loss2) and torch.equal(d, d2)
    # gamma = 0 with unit weights is cross-entropy (q^0 = exp(-0 x) = 1 exactly)
    loss3, d3 = ops.ce_loss(zt, yt, focal_gamma=0.0)
    assert torch.equal(loss, loss3) and float((d - d3).abs().max()) * n <= U


def test_minus_100_is_a_bad_label_by_default_and_ignored_under_any_option():
    z, y = trainer_ref.ce_inputs(64, seed=2)
    y = y.copy()
    y[5] = -100
    zt, yt = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
    stats = ops.new_loss_stats(DEV)
    ops.ce_loss(zt, yt, stats)
    assert ops.read_loss_stats(stats)["bad_labels"] == 1
    stats.zero_()
    loss, _ = ops.ce_loss(zt, yt, stats, weight=(1.0, 1.0))
    assert ops.read_loss_stats(stats)["bad_labels"] == 0
    keep = y != -100
    l64 = trainer_ref.ce(z[keep], y[keep])[0]                                    # the mean over the 63 that count
    assert abs(float(loss) - l64) <= U * l64


def test_stats_accumulate_batch_sums_under_a_sum_reduction():
    stats = ops.new_loss_stats(DEV)
    want = 0.0
    for n in (5, 64):
        z, y = ref.case_inputs(n, "mixed")
        loss, _ = ops.ce_loss(torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV), stats, weight=(0.25, 4.0), reduction="sum")
        want += float(loss)
    s = ops.read_loss_stats(stats)
    assert s["loss_sum"] == want and s["batches"] == 2 and s["total"] == 69


def test_ops_refuse_bad_options_before_any_launch():
    z = torch.zeros(4, 2, device=DEV)
    y = torch.zeros(4, dtype=torch.int64, device=DEV)
    d = torch.full((4, 2), GUARD, device=DEV)
    for kw in (dict(weight=(1.0,)), dict(weight=(1.0, -1.0)), dict(weight=torch.ones(3, device=DEV)), dict(label_smoothing=1.5),
               dict(reduction="max"), dict(focal_gamma=-1.0), dict(focal_gamma=2.0, label_smoothing=0.125), dict(ignore_index=1.5)):
        with pytest.raises(ValueError):
            ops.ce_loss_into(z, y, d, None, None, **kw)
    with pytest.raises(NotImplementedError):
        ops.ce_loss(z, y, reduction="none")
    assert torch.all(d == GUARD)
    loss, _ = ops.ce_loss(z, y, weight=torch.tensor([0.25, 4.0], device=DEV))     # a weight tensor on the device is read once, here
    assert abs(float(loss) - np.log(2.0)) <= U


# ======================================================================================================================================
# trainer
# ======================================================================================================================================
B = 16
MODELS = {"simple": pkg.SimpleWakewordModel, "full": pkg.WakewordModel}
W = (0.25, 4.0)


def _criterion(kind):
    w = torch.tensor(W, device=DEV)
    if kind == "ce":
        return nn.CrossEntropyLoss(weight=w, label_smoothing=0.125), dict(weight=W, label_smoothing=0.125)
    return pkg.FocalLoss(2.0, weight=w), dict(weight=W, focal_gamma=2.0)


def _batch(n, T, seed):
    g = torch.Generator().manual_seed(seed)
    x = (-40.0 + 20.0 * torch.randn(n, 1, 80, T, generator=g)).to(DEV)
    y = torch.randint(0, 2, (n, 1), generator=g).to(DEV)
    return x, y


def _model(name, seed=1234):
    torch.manual_seed(seed)
    return MODELS[name]().to(DEV)


@pytest.mark.parametrize("kind", ["ce", "focal"])
@pytest.mark.parametrize("name, T", [("simple", 8), ("full", 8), ("simple", 32)])
def test_trainer_computes_the_criterion_it_holds(name, T, kind):
    crit, opts = _criterion(kind)
    cap_loss, cap_d = _caps(opts)
    model, twin = _model(name), _model(name)
    trainer = pkg.WakewordTrainer(model, DEV)
    trainer.criterion = crit
    assert trainer.criterion is crit
    model.train(); twin.train()
    x, y = _batch(B, T, seed=3)
    torch.manual_seed(77)
    trainer.step(x, y)
    # ---- d loss / d logits: torch's autograd of the criterion on the step's own logits is the reference ----
    logits = trainer.last_logits[:B].clone()
    zr = logits.clone().requires_grad_()
    lt = crit(zr, y[:, 0])
    lt.backward()
    want = ref.loss(_np(logits), _np(y)[:, 0], W, opts.get("label_smoothing", 0.0), -100, "mean", opts.get("focal_gamma"))
    _rule(f"{name} T={T} {kind} dlogits", ref.dlogits_error(_np(trainer._dlogits[:B]), want), ref.dlogits_error(_np(zr.grad), want), cap_d)
    _rule(f"{name} T={T} {kind} loss", ref.loss_error(float(trainer.last_loss), want["loss"]), ref.loss_error(float(lt.detach()), want["loss"]), cap_loss)
    # ---- the parameter gradients: autograd through the same kernels, fed this loss's d loss / d logits (section 3h's identity) ----
    torch.manual_seed(77)
    out = twin(x)
    assert torch.equal(out.detach(), logits)
    out.backward(gradient=ops.ce_loss(out.detach(), y, **opts)[1])
    tnamed = dict(twin.named_parameters())
    for k, p in model.named_parameters():
        assert torch.equal(p.grad, tnamed[k].grad), k
    # ---- validate: the mean over batches of the torch criterion on the same logits ----
    xv, yv = _batch(37, T, seed=8)
    batches = [(xv[i:i + 16], yv[i:i + 16]) for i in range(0, 37, 16)]
    vloss, _ = trainer.validate(batches)
    hand, h64 = 0.0, 0.0
    with torch.no_grad():
        for xb, yb in batches:
            o = model(xb)
            hand += float(crit(o, yb[:, 0]))
            h64 += ref.loss(_np(o), _np(yb)[:, 0], W, opts.get("label_smoothing", 0.0), -100, "mean", opts.get("focal_gamma"))["loss"]
    _rule(f"{name} T={T} {kind} validate loss", abs(vloss - h64 / 3) / (h64 / 3), abs(hand / 3 - h64 / 3) / (h64 / 3), cap_loss)
    # ---- a step has no hidden wait and allocates nothing ----
    model.train()
    y1 = y.contiguous()
    trainer.step(x, y1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        trainer.step(x, y1)
        before = torch.cuda.memory_allocated()
        trainer.step(x, y1)
        after = torch.cuda.memory_allocated()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert before == after


@pytest.mark.parametrize("kind", ["ce", "focal"])
def test_minus_100_labels_do_not_raise_under_these_criteria(kind):
    crit, _ = _criterion(kind)
    model = _model("simple")
    trainer = pkg.WakewordTrainer(model, DEV, criterion=crit)                        # the constructor's keyword
    assert trainer.criterion is crit
    x, y = _batch(B, 8, seed=5)
    y = y.clone()
    y[3] = -100
    torch.manual_seed(1)
    loss, acc = trainer.train_epoch([(x, y)])
    assert loss == loss and trainer._dlogits[3].abs().max() == 0.0
    vloss, vacc = trainer.validate([(x, y)])
    assert vloss == vloss and vacc <= 100.0 * 15 / 16                                # the ignored clip counts as wrong, as in the reference's loop
    bad = y.clone()
    bad[4] = 7
    with pytest.raises(ValueError, match="labels"):                                  # another label outside {0, 1} is still an error
        trainer.validate([(x, bad)])
    plain = pkg.WakewordTrainer(_model("simple"), DEV)
    with pytest.raises(ValueError, match="labels"):                                  # and -100 still is one under the default criterion
        plain.validate([(x, y)])


def test_criterion_is_checked_at_the_assignment():
    trainer = pkg.WakewordTrainer(_model("simple"), DEV)
    held = trainer.criterion
    assert isinstance(held, nn.CrossEntropyLoss) and trainer._loss_opts is None
    with pytest.raises(TypeError):
        trainer.criterion = nn.MSELoss()
    with pytest.raises(TypeError):
        trainer.criterion = nn.BCEWithLogitsLoss()
    with pytest.raises(NotImplementedError):
        trainer.criterion = nn.CrossEntropyLoss(reduction="none")
    with pytest.raises(NotImplementedError):
        trainer.criterion = pkg.FocalLoss(reduction="none")
    with pytest.raises(ValueError):
        trainer.criterion = nn.CrossEntropyLoss(weight=torch.ones(3, device=DEV))
    with pytest.raises(TypeError):
        pkg.WakewordTrainer(_model("simple"), DEV, criterion=nn.MSELoss())
    assert trainer.criterion is held                                                 # a refused assignment changes nothing
    trainer.criterion = nn.CrossEntropyLoss(reduction="sum")
    assert trainer._loss_opts is not None and trainer._loss_opts.reduction == 1


def test_a_default_criterion_assigned_again_is_the_plain_step():
    x, y = _batch(B, 8, seed=3)
    models = [_model("simple"), _model("simple")]
    trainers = [pkg.WakewordTrainer(m, DEV) for m in models]
    trainers[1].criterion = nn.CrossEntropyLoss()
    assert trainers[1]._loss_opts is None
    for m, t in zip(models, trainers):
        m.train()
        torch.manual_seed(77)
        t.step(x, y)
    assert torch.equal(trainers[0].last_loss, trainers[1].last_loss) and torch.equal(trainers[0]._dlogits, trainers[1]._dlogits)
    for p, q in zip(models[0].parameters(), models[1].parameters()):
        assert torch.equal(p, q)


def test_focal_loss_module_on_the_device_matches_the_kernel():
    z, y = ref.case_inputs(257, "mixed")
    zt, yt = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
    crit = pkg.FocalLoss(2.0, weight=torch.tensor(W)).to(DEV)
    want = ref.loss(z, y, W, focal_gamma=2.0)
    loss, _ = ops.ce_loss(zt, yt, weight=W, focal_gamma=2.0)
    _rule("FocalLoss module", ref.loss_error(float(loss), want["loss"]), ref.loss_error(float(crit(zt, yt)), want["loss"]), ref.CAP_FOCAL_LOSS)
