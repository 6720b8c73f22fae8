"""Knowledge distillation without a GPU: loss.DistillationLoss against the float64 restatement of
tests/distill_ref.py and against torch's own composition (F.cross_entropy + F.kl_div(..., "batchmean") * T^2) in float64, autograd
gradients included; its two limits (alpha = 0, and alpha = 1 at T = 1); the C entry's binding and its refusals before any HIP call; and
the argument refusals of DistillationLoss, ops.distill_loss and WakewordTrainer that need no device.

Float64 against float64: rtol 1e-12 (the two sides order their sums differently), with an absolute 1e-14 for gradient elements that
cancel: p - onehot and p - q carry the 2.2e-16 of a float64 softmax, times a class weight of up to 4 or alpha T of up to 20 under the sum.
A loss gets the absolute 1e-12 of the issue's own bound: a KD term that cancels to zero (teacher and student tied) keeps T^2 = 400 times
the 2.2e-16 of its log-softmaxes."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import distill_ref as ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import ops
from wakeword_jupyterlab_amd.loss import DistillationLoss, FocalLoss

L = nat.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-12, 1e-14


def _err():
    return (L.ww_last_error() or b"").decode()


def _criterion(opts):
    w = None if opts.get("weight") is None else torch.tensor(opts["weight"], dtype=torch.float64)
    if opts.get("focal_gamma") is not None:
        return FocalLoss(opts["focal_gamma"], weight=w, reduction=opts.get("reduction", "mean"), ignore_index=opts.get("ignore_index", -100))
    return nn.CrossEntropyLoss(weight=w, label_smoothing=opts.get("label_smoothing", 0.0), ignore_index=opts.get("ignore_index", -100),
                               reduction=opts.get("reduction", "mean"))


def _module(z, zt, target, alpha, T, opts):
    """(loss, gradient) of DistillationLoss in float64 with autograd."""
    zz = torch.from_numpy(z).double().requires_grad_()
    tg = None if target is None else torch.from_numpy(np.asarray(target))
    loss = DistillationLoss(alpha, T, _criterion(opts))(zz, torch.from_numpy(zt).double(), tg)
    loss.backward()
    return float(loss.detach()), zz.grad.numpy()


def _close(a, b):
    return np.allclose(a, b, rtol=RTOL, atol=1e-12 if np.ndim(a) == 0 else ATOL, equal_nan=True)


# ---- the module --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 3, 257))
def test_distillation_loss_matches_the_restatement(n):
    z, zt, y, t = ref.inputs(n)
    for tag, kind, opts, alpha, T in ref.grid():
        target = ref.target_of(kind, y, t)
        want = ref.distill(z, zt, target, alpha, T, **opts)
        loss, grad = _module(z, zt, target, alpha, T, opts)
        assert _close(loss, want["loss"]), f"{tag} n={n}: {loss!r} against {want['loss']!r}"
        assert _close(grad, want["dlogits"]), f"{tag} n={n}"


@pytest.mark.parametrize("n", (2, 65))
def test_distillation_loss_matches_torchs_own_composition(n):
    z, zt, y, t = ref.inputs(n, nonfinite_teacher=False)
    y = np.where((y == 0) | (y == 1) | (y == -100), y, -100)                         # torch refuses a label 7
    t[~np.isfinite(t).all(axis=1)] = (0.25, 0.75)                                    # and has no rule for a NaN row
    for T in ref.TEMPERATURES:
        for alpha in ref.ALPHAS:
            for target, kw in ((y, {}), (y, dict(weight=(0.25, 4.0), label_smoothing=0.125)), (t, {}), (t, dict(weight=(0.25, 4.0)))):
                w = None if "weight" not in kw else torch.tensor(kw["weight"], dtype=torch.float64)
                zz = torch.from_numpy(z).double().requires_grad_()
                tg = torch.from_numpy(target).double() if target.dtype.kind == "f" else torch.from_numpy(target)
                hard = F.cross_entropy(zz, tg, weight=w, label_smoothing=kw.get("label_smoothing", 0.0))
                kd = F.kl_div(F.log_softmax(zz / T, dim=1), F.softmax(torch.from_numpy(zt).double() / T, dim=1), reduction="batchmean") * T * T
                total = (1.0 - alpha) * hard + alpha * kd
                total.backward()
                loss, grad = _module(z, zt, target, alpha, T, kw)
                assert _close(loss, float(total.detach())), (T, alpha, kw)
                assert _close(grad, zz.grad.numpy()), (T, alpha, kw)


def test_alpha_zero_is_the_criterion():
    z, zt, y, t = ref.inputs(65, nonfinite_teacher=False)
    y = np.where((y == 0) | (y == 1) | (y == -100), y, -100)
    for opts in (dict(), dict(weight=(0.25, 4.0), label_smoothing=0.125), dict(reduction="sum"), dict(focal_gamma=2.0, weight=(0.25, 4.0))):
        crit = _criterion(opts)
        zz = torch.from_numpy(z).double().requires_grad_()
        want = crit(zz, torch.from_numpy(y))
        want.backward()
        loss, grad = _module(z, zt, y, 0.0, 3.0, opts)
        assert _close(loss, float(want.detach())) and _close(grad, zz.grad.numpy()), opts


def test_alpha_one_at_unit_temperature_is_soft_cross_entropy_minus_the_teachers_entropy():
    z, zt, y, _ = ref.inputs(65, nonfinite_teacher=False)
    zz = torch.from_numpy(z).double().requires_grad_()
    q = F.softmax(torch.from_numpy(zt).double(), dim=1)
    entropy = -(q * F.log_softmax(torch.from_numpy(zt).double(), dim=1)).sum(dim=1).mean()
    want = F.cross_entropy(zz, q) - entropy
    want.backward()
    loss, grad = _module(z, zt, y, 1.0, 1.0, {})
    assert _close(grad, zz.grad.numpy())
    # the difference of two sums of this size cancels: the bound is relative to the cross-entropy, not to the difference
    assert abs(loss - float(want.detach())) <= RTOL * float(F.cross_entropy(zz, q).detach())


def test_empty_terms_and_no_gradient_to_the_teacher():
    z, zt, y, _ = ref.inputs(9, nonfinite_teacher=False)
    zz = torch.from_numpy(z).double().requires_grad_()
    tt = torch.from_numpy(zt).double().requires_grad_()
    DistillationLoss(0.3, 2.0)(zz, tt, torch.from_numpy(np.where(y == 7, -100, y))).backward()
    assert tt.grad is None and zz.grad is not None
    nans = torch.full((9, 2), float("nan"), dtype=torch.float64)
    zz = torch.from_numpy(z).double().requires_grad_()
    loss = DistillationLoss(0.3, 2.0)(zz, nans, torch.full((9,), -100))
    loss.backward()
    assert bool(torch.isnan(loss.detach())) and not zz.grad.any()                       # nothing counted: NaN, a gradient of zeros
    zz = torch.from_numpy(z).double().requires_grad_()
    loss = DistillationLoss(0.3, 2.0)(zz, nans, torch.from_numpy(np.where(y == 7, -100, y)))      # the hard term alone, a finite loss
    want = 0.7 * F.cross_entropy(torch.from_numpy(z).double(), torch.from_numpy(np.where(y == 7, -100, y)))
    assert _close(float(loss.detach()), float(want))


def test_distillation_loss_refusals():
    for kw in (dict(alpha=-0.1), dict(alpha=1.1), dict(alpha=float("nan")), dict(alpha=True), dict(temperature=0.0), dict(temperature=-2.0),
               dict(temperature=float("inf")), dict(temperature=float("nan")), dict(temperature="2")):
        with pytest.raises(ValueError):
            DistillationLoss(**kw)
    with pytest.raises(TypeError):
        DistillationLoss(criterion=nn.MSELoss())
    with pytest.raises(NotImplementedError):
        DistillationLoss(criterion=nn.CrossEntropyLoss(reduction="none"))
    z, t = torch.zeros(4, 2), torch.full((4, 2), 0.5)
    with pytest.raises(ValueError):
        DistillationLoss()(z, torch.zeros(3, 2), None)
    with pytest.raises(ValueError):
        DistillationLoss()(torch.zeros(4, 3), torch.zeros(4, 3), None)
    with pytest.raises(ValueError):
        DistillationLoss()(z, z, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(NotImplementedError):
        DistillationLoss(criterion=FocalLoss(2.0))(z, z, t)
    with pytest.raises(ValueError):
        DistillationLoss(criterion=nn.CrossEntropyLoss(ignore_index=1))(z, z, t)


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_bound_and_the_abi_stays_4():
    assert L.ww_abi_version() == 4 == nat.ABI_VERSION
    assert nat.PROTOTYPES["ww_distill_loss_f32"] == (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int64, C.POINTER(nat.LossOpts), C.c_double, C.c_double]
                                                     + [C.c_void_p] * 5)
    assert L.ww_distill_loss_f32.argtypes == nat.PROTOTYPES["ww_distill_loss_f32"][1]
    assert C.sizeof(nat.DistillStats) == 64 == 8 * len(ops.DISTILL_STATS_FIELDS)
    assert [f[0] for f in nat.DistillStats._fields_] == list(ops.DISTILL_STATS_FIELDS)
    text = open(os.path.join(ROOT, "include", "wakeword_amd.h")).read()
    body = re.search(r"typedef struct ww_distill_stats \{(.*?)\} ww_distill_stats;", text, flags=re.S).group(1)
    assert re.findall(r"(?:double|int64_t)\s+(\w+);", body) == list(ops.DISTILL_STATS_FIELDS)
    assert (nat.TARGET_LABELS, nat.TARGET_PROBS) == tuple(int(re.search(rf"#define WW_TARGET_{k} (\d+)", text).group(1)) for k in ("LABELS", "PROBS"))


def _call(logits=16, teacher=32, targets=48, kind=0, n=4, opts=None, alpha=0.5, T=2.0, dlogits=None, loss=None, stats=None, dstats=None):
    return L.ww_distill_loss_f32(logits, teacher, targets, kind, n, None if opts is None else C.byref(opts), alpha, T, dlogits, loss, stats, dstats,
                                 None)


def _opts(**kw):
    o = nat.LossOpts()
    o.class_weight[0], o.class_weight[1] = kw.pop("w", (1.0, 1.0))
    o.label_smoothing, o.focal_gamma, o.ignore_index, o.kind, o.reduction = 0.0, 0.0, -100, nat.LOSS_CE, nat.REDUCE_MEAN
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("kw, word", [
    (dict(alpha=-0.5), "alpha"), (dict(alpha=1.5), "alpha"), (dict(alpha=float("nan")), "alpha"),
    (dict(T=0.0), "temperature"), (dict(T=-1.0), "temperature"), (dict(T=float("inf")), "temperature"), (dict(T=float("nan")), "temperature"),
    (dict(teacher=None), "teacher"), (dict(teacher=34), "teacher_logits_dev"), (dict(dstats=4), "distill_stats_dev"),
    (dict(kind=2), "target_kind"), (dict(kind=-1), "target_kind"),
    (dict(n=0), "n 0"), (dict(n=2 ** 30 + 1), "n "), (dict(logits=None), "null logits"), (dict(logits=18), "4-byte"),
    (dict(targets=52), "8-byte"), (dict(kind=1, targets=50), "4-byte"), (dict(stats=4), "8-byte"), (dict(dlogits=2), "4-byte"),
    (dict(opts=_opts(w=(-1.0, 1.0))), "class_weight[0]"), (dict(opts=_opts(label_smoothing=2.0)), "label_smoothing"),
    (dict(opts=_opts(reduction=3)), "reduction"), (dict(opts=_opts(kind=nat.LOSS_FOCAL, label_smoothing=0.5)), "label_smoothing"),
    (dict(kind=1, opts=_opts(kind=nat.LOSS_FOCAL)), "kind"), (dict(kind=1, opts=_opts(ignore_index=1)), "ignore_index"),
    (dict(targets=None, opts=_opts(reduction=3)), "reduction"), (dict(targets=None, n=0), "n 0"), (dict(targets=None, logits=None), "null logits"),
    (dict(targets=None, stats=4), "8-byte"),
])
def test_the_entry_refuses_bad_arguments_before_any_hip_call(kw, word):
    """The device pointers are small made-up addresses that are never dereferenced: the field is named, so the check ran on the host."""
    assert _call(**kw) == nat.WW_EINVAL and word in _err(), _err()


# ---- the Python surface --------------------------------------------------------------------------------------------------------------
def test_ops_refusals_without_a_device():
    z, y = torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64)
    for kw in (dict(alpha=2.0), dict(temperature=0.0), dict(weight=(1.0,)), dict(reduction="max"), dict(label_smoothing=3.0)):
        with pytest.raises(ValueError):
            ops.distill_loss(z, z, y, **kw)
    with pytest.raises(NotImplementedError):
        ops.distill_loss(z, z, y, reduction="none")
    with pytest.raises(NotImplementedError):
        ops.distill_loss(z, z, torch.zeros(4, 2), focal_gamma=2.0)
    with pytest.raises(TypeError):
        ops.distill_loss(z, z, [0, 1, 0, 1])
    with pytest.raises(RuntimeError, match="CPU"):
        ops.distill_loss(z, z, y)                                                   # good arguments, no device: no quiet fall-back
    with pytest.raises(RuntimeError, match="CPU"):
        ops.new_distill_stats("cpu")
    host = torch.zeros(8, dtype=torch.int64)
    host[:2] = torch.tensor([1.5, 2.25], dtype=torch.float64).view(torch.int64)
    host[2:] = torch.arange(1, 7)
    assert ops.read_distill_stats(host) == {"hard_sum": 1.5, "kd_sum": 2.25, "kd_rows": 1, "hard_rows": 2, "agree": 3, "teacher_correct": 4,
                                            "teacher_nonfinite": 5, "batches": 6}


def test_trainer_refusals_without_a_device():
    student, teacher = pkg.SimpleWakewordModel(), pkg.WakewordModel().eval()
    for kw in (dict(distill_alpha=1.5), dict(distill_alpha=-1.0), dict(distill_temperature=0.0), dict(distill_temperature=float("inf"))):
        with pytest.raises(ValueError):
            pkg.WakewordTrainer(student, "cpu", teacher=teacher, **kw)
    with pytest.raises(ValueError, match="teacher"):
        pkg.WakewordTrainer(student, "cpu", teacher=student)
    with pytest.raises(TypeError, match="teacher"):
        pkg.WakewordTrainer(student, "cpu", teacher=nn.Linear(2, 2))
    with pytest.raises(RuntimeError, match="eval"):
        pkg.WakewordTrainer(student, "cpu", teacher=pkg.WakewordModel())            # a fresh module is in train mode
    shared = pkg.SimpleWakewordModel().eval()
    shared.fc.weight = student.fc.weight                                             # a trainable parameter that IS the student's
    with pytest.raises(ValueError, match="storage"):
        pkg.WakewordTrainer(student, "cpu", teacher=shared)
    with pytest.raises(TypeError, match="CPU"):                                      # a good teacher: the next refusal is the old one
        pkg.WakewordTrainer(student, "cpu", teacher=teacher)
