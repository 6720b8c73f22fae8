"""WakewordTrainer, FusedAdam and their three kernels on the GPU (csrc/ww_optim.hip).

Tolerances (tests/trainer_ref.py): the reference for every float32 quantity is torch's own float32 result on the same device and inputs;
its error against the float64 restatement is measured here and must stay under a fixed cap; ours may be at most twice that plus 2^-24.
Shapes: B = 16, T = 8 (0.25 s) plus one case at T = 32, for both models."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import trainer_ref as ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = ref.U


def _np(t):
    return t.detach().cpu().numpy()


def _rule(name, ours, torchs, cap):
    """`ours` and `torchs` are error figures against float64: the reference stays under its cap, ours under twice the reference + 2^-24."""
    print(f"{name}: ours {ours / U:.3f} u, torch {torchs / U:.3f} u (u = 2^-24)")
    assert torchs <= cap, f"{name}: the reference's own error {torchs / U:.3f} u exceeds its cap {cap / U:.1f} u"
    assert ours <= ref.allowed(torchs), f"{name}: {ours / U:.3f} u > 2 x {torchs / U:.3f} u + 1 u"


# ======================================================================================================================================
# loss kernel
# ======================================================================================================================================
def _ce_case(z, y):
    zt, yt = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
    stats = ops.new_loss_stats(DEV)
    loss, d = ops.ce_loss(zt, yt, stats)
    zr = zt.clone().requires_grad_()
    lr = F.cross_entropy(zr, yt)
    lr.backward()
    l64, d64, c64 = ref.ce(z, y)
    n = len(y)
    _rule(f"loss n={n}", abs(float(loss) - l64) / abs(l64), abs(float(lr.detach()) - l64) / abs(l64), ref.CAP_LOSS)
    _rule(f"dlogits n={n}", float(np.abs(_np(d).astype(np.float64) - d64).max()) * n, float(np.abs(_np(zr.grad).astype(np.float64) - d64).max()) * n,
          ref.CAP_DLOGITS)
    s = ops.read_loss_stats(stats)
    assert (s["correct"], s["total"], s["batches"], s["bad_labels"], s["nonfinite"]) == (c64, n, 1, 0, 0)
    assert s["correct"] == int((torch.max(zt, 1)[1] == yt).sum())
    assert s["loss_sum"] == float(loss)
    return zt, yt, loss, d


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 4099])
def test_ce_loss_against_float64(n):
    z, y = ref.ce_inputs(n, seed=n)
    zt, yt, loss, d = _ce_case(z, y)
    loss2, d2 = ops.ce_loss(zt, yt)                                # a second run is bit-equal
    assert torch.equal(loss, loss2) and torch.equal(d, d2)
    # pointers off the 16-byte grid (4-byte aligned logits and gradient): the same bits
    buf = torch.zeros(2 * n + 1, device=DEV)
    buf[1:] = zt.reshape(-1)
    stats = ops.new_loss_stats(DEV)
    loss3 = torch.empty((), device=DEV)
    d3 = torch.full((2 * n + 2,), 7.0, device=DEV)
    ops.ce_loss_into(buf[1:].view(n, 2), yt, d3[1:2 * n + 1].view(n, 2), loss3, stats)
    assert torch.equal(loss3, loss) and torch.equal(d3[1:2 * n + 1].view(n, 2), d) and d3[0] == 7.0 and d3[-1] == 7.0


@pytest.mark.parametrize("labels", ["zeros", "ones"])
def test_ce_loss_with_one_class_only(labels):
    _ce_case(*ref.ce_inputs(257, seed=9, labels=labels))


def test_ce_loss_stats_accumulate_and_the_validation_form_writes_no_gradient():
    stats = ops.new_loss_stats(DEV)
    want_sum, want_correct, want_total = 0.0, 0, 0
    for n in (5, 64, 1001):
        z, y = ref.ce_inputs(n, seed=100 + n)
        # logits, then a canary where a gradient would go if the kernel wrote one
        buf = torch.full((4 * n,), 123.0, device=DEV)
        buf[:2 * n] = torch.from_numpy(z).to(DEV).reshape(-1)
        loss = torch.empty((), device=DEV)
        ops.ce_loss_into(buf[:2 * n].view(n, 2), torch.from_numpy(y).to(DEV), None, loss, stats)
        assert torch.all(buf[2 * n:] == 123.0)
        want_sum += float(loss)                                    # the sum of the batch means, as `running_loss += loss.item()`
        want_correct += ref.ce(z, y)[2]
        want_total += n
        assert abs(float(loss) - ref.ce(z, y)[0]) <= U * abs(ref.ce(z, y)[0])       # float64 inside, rounded once
    s = ops.read_loss_stats(stats)
    assert s == {"loss_sum": want_sum, "correct": want_correct, "total": want_total, "batches": 3, "bad_labels": 0, "nonfinite": 0}
    loss, d = ops.ce_loss(buf[:2 * n].view(n, 2), torch.from_numpy(y).to(DEV).view(n, 1), grad=False)      # [n, 1] targets; no gradient asked
    assert d is None


def test_ce_loss_counts_bad_labels_and_nonfinite_logits():
    z, y = ref.ce_inputs(130, seed=4)
    y2 = y.copy()
    y2[7], y2[64], y2[129] = 2, -1, 2
    stats = ops.new_loss_stats(DEV)
    loss, d = ops.ce_loss(torch.from_numpy(z).to(DEV), torch.from_numpy(y2).to(DEV), stats)
    l64, d64, c64 = ref.ce(z, y2)
    s = ops.read_loss_stats(stats)
    assert (s["bad_labels"], s["nonfinite"], s["correct"], s["total"]) == (3, 0, c64, 130)
    assert torch.all(d[[7, 64, 129]] == 0.0)                       # exact zeros
    assert abs(float(loss) - l64) <= U * abs(l64)                  # float64 inside, one rounding: the rest's loss over the same n
    assert float(np.abs(_np(d).astype(np.float64) - d64).max()) * 130 <= U
    z2 = z.copy()
    z2[11, 0], z2[12, 1], z2[100, 0] = np.inf, -np.inf, np.nan
    stats.zero_()
    ops.ce_loss(torch.from_numpy(z2).to(DEV), torch.from_numpy(y).to(DEV), stats)
    s = ops.read_loss_stats(stats)
    assert (s["bad_labels"], s["nonfinite"], s["total"]) == (0, 3, 130)


def test_ops_argument_checks():
    z = torch.zeros(4, 2, device=DEV)
    y = torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError):
        ops.ce_loss(z.cpu(), y)
    with pytest.raises(TypeError):
        ops.ce_loss(z, y.int())
    with pytest.raises(ValueError):
        ops.ce_loss(z, y[:3])
    with pytest.raises(ValueError):
        ops.ce_loss(torch.zeros(4, 3, device=DEV), y)
    with pytest.raises(TypeError):
        ops.ce_loss(z, y, stats=torch.zeros(6, device=DEV))
    with pytest.raises(ValueError):
        ops.grad_norm([z] * 17, 1.0)
    with pytest.raises(RuntimeError):
        ops.grad_norm([z.t()], 1.0)
    with pytest.raises(nat.NativeError, match="max_norm"):
        ops.grad_norm([z], 0.0)


# ======================================================================================================================================
# Adam kernel
# ======================================================================================================================================
SIZES = [1, 2, 3, 4, 5, 255, 256, 257, 65536, 262145, 3, 257, 255, 5, 1000, 1000]       # 16 tensors; the last two share one gradient
# phase of each view on the 16-byte grid, in floats, for (p, g, m, v): equal phases take the vector path with a scalar head and tail,
# unequal ones the scalar path
PHASES = [(0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0), (1, 1, 1, 1), (3, 3, 3, 3), (1, 1, 1, 1), (0, 0, 0, 0), (2, 2, 2, 2), (0, 0, 0, 0),
          (1, 1, 1, 1), (0, 1, 0, 0), (1, 0, 2, 3), (0, 0, 0, 1), (2, 2, 2, 2), (1, 1, 1, 1), (1, 1, 1, 1)]
GUARD = 8
GUARD_VALUE = -77.25


class _Views:
    """16 views per role (p, g, m, v) cut from one buffer per role, guard words between and around them."""

    def __init__(self, seed, share_last_g=True):
        self.off = {r: [] for r in range(4)}
        total = [GUARD] * 4
        for n, ph in zip(SIZES, PHASES):
            for r in range(4):
                start = -(-total[r] // 4) * 4 + ph[r]
                self.off[r].append(start)
                total[r] = start + n + GUARD
        self.buf = [torch.full((total[r] + 4,), GUARD_VALUE, device=DEV) for r in range(4)]
        assert all(b.data_ptr() % 16 == 0 for b in self.buf)
        self.p0, self.gs = [], []
        for k, n in enumerate(SIZES):
            p0, gs = ref.adam_inputs(n, seed=seed + k)
            if share_last_g and k == 15:
                gs = self.gs[14]
            self.p0.append(p0)
            self.gs.append(gs)
            self.view(0, k).copy_(torch.from_numpy(p0))
            self.view(2, k).zero_()
            self.view(3, k).zero_()
        if share_last_g:
            self.off[1][15] = self.off[1][14]

    def view(self, role, k):
        return self.buf[role][self.off[role][k]:self.off[role][k] + SIZES[k]]

    def views(self, role):
        return [self.view(role, k) for k in range(16)]

    def set_grads(self, t, mul=1.0):
        for k in range(16):
            self.view(1, k).copy_(torch.from_numpy(self.gs[k][t] * np.float32(mul)))

    def guards_intact(self):
        for r in range(4):
            mask = torch.ones_like(self.buf[r], dtype=torch.bool)
            for k in range(16):
                mask[self.off[r][k]:self.off[r][k] + SIZES[k]] = False
            if not torch.all(self.buf[r][mask] == GUARD_VALUE):
                return False
        return True

    def cat(self, role):
        return np.concatenate([_np(self.view(role, k)) for k in range(16)])


def _torch_adam_run(v, lr, wd, steps, mul=1.0):
    """torch's single-tensor Adam on the same device over contiguous copies of the 16 tensors: (p, m, v) concatenated, after `steps`."""
    params = [torch.nn.Parameter(torch.from_numpy(p0).to(DEV)) for p0 in v.p0]
    opt = torch.optim.Adam(params, lr=lr, weight_decay=wd, foreach=False)
    for t in range(steps):
        for k, p in enumerate(params):
            p.grad = torch.from_numpy(v.gs[k][t] * np.float32(mul)).to(DEV)
        opt.step()
    return (np.concatenate([_np(p) for p in params]), np.concatenate([_np(opt.state[p]["exp_avg"]) for p in params]),
            np.concatenate([_np(opt.state[p]["exp_avg_sq"]) for p in params]))


def _f64_adam_run(v, lr, wd, steps, scale=1.0):
    p = np.concatenate(v.p0).astype(np.float64)
    m, s = np.zeros_like(p), np.zeros_like(p)
    gmax = 0.0
    for t in range(steps):
        g = np.concatenate([v.gs[k][t] for k in range(16)])
        p, m, s, g1 = ref.adam_step(p, g, m, s, lr, 0.9, 0.999, 1e-8, wd, t + 1, scale)
        gmax = max(gmax, float(np.abs(g1).max()))
    return p, m, s, gmax


def _adam_rule(tag, ours, torchs, f64, lr):
    p64, m64, v64, gmax = f64
    eo, et = ref.adam_errors(*ours, p64, m64, v64, lr, gmax), ref.adam_errors(*torchs, p64, m64, v64, lr, gmax)
    for name, o, t, cap in zip("pmv", eo, et, (ref.CAP_P, ref.CAP_M, ref.CAP_V)):
        _rule(f"{tag} {name}", o, t, cap)


@pytest.mark.parametrize("lr", [1e-4, 1e-3])
@pytest.mark.parametrize("wd", [0.0, 1e-5])
def test_adam_kernel_16_tensors_3_steps(lr, wd):
    v = _Views(seed=40)
    for t in range(3):
        v.set_grads(t)
        ops.adam_step(v.views(0), v.views(1), v.views(2), v.views(3), lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, step=t + 1)
    assert v.guards_intact()
    _adam_rule(f"adam lr={lr} wd={wd}", (v.cat(0), v.cat(2), v.cat(3)), _torch_adam_run(v, lr, wd, 3), _f64_adam_run(v, lr, wd, 3), lr)
    # the two entries that share one gradient behave as two copies: same g, their own p
    assert not np.array_equal(_np(v.view(0, 14)), _np(v.view(0, 15))) and np.array_equal(_np(v.view(3, 14)) > 0, _np(v.view(3, 15)) > 0)


def test_adam_kernel_grad_scale_equals_prescaled_gradients():
    lr, wd, scale = 1e-3, 1e-5, 0.25                               # a power of two: pre-scaling in float32 is exact
    v = _Views(seed=60)
    st = torch.tensor([scale], device=DEV)
    for t in range(3):
        v.set_grads(t)
        ops.adam_step(v.views(0), v.views(1), v.views(2), v.views(3), lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, step=t + 1, grad_scale=st)
    assert v.guards_intact()
    _adam_rule("adam grad_scale", (v.cat(0), v.cat(2), v.cat(3)), _torch_adam_run(v, lr, wd, 3, mul=scale), _f64_adam_run(v, lr, wd, 3, scale), lr)
    w = _Views(seed=60)
    for t in range(3):
        w.set_grads(t, mul=scale)
        ops.adam_step(w.views(0), w.views(1), w.views(2), w.views(3), lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, step=t + 1)
    assert np.array_equal(v.cat(0), w.cat(0)) and np.array_equal(v.cat(3), w.cat(3))


def _params17(seed):
    out = []
    for k in range(17):
        p0, gs = ref.adam_inputs([5, 300, 4097][k % 3], seed=seed + k)
        p = torch.nn.Parameter(torch.from_numpy(p0).to(DEV))
        out.append((p, [torch.from_numpy(g).to(DEV) for g in gs]))
    return out


def test_fused_adam_17_parameters_are_two_launches(monkeypatch):
    calls = []
    real = ops.adam_launch
    monkeypatch.setattr(ops, "adam_launch", lambda table, *a, **k: (calls.append(len(table)), real(table, *a, **k))[1])
    many, single = _params17(7), _params17(7)
    opt = pkg.FusedAdam([p for p, _ in many], lr=1e-3, weight_decay=1e-5)
    singles = [pkg.FusedAdam([p], lr=1e-3, weight_decay=1e-5) for p, _ in single]
    for t in range(3):
        for p, gs in many + single:
            p.grad = gs[t]
        del calls[:]
        opt.step()
        assert calls == [16, 1]
        for o in singles:
            o.step()
    for i, ((p, _), (q, _)) in enumerate(zip(many, single)):
        assert torch.equal(p, q) and p._version == 3
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[p][key], singles[i].state[q][key])
    assert float(opt.state[many[0][0]]["step"]) == 3.0 and opt.state[many[0][0]]["step"].device.type == "cpu"


def test_fused_adam_refuses_what_the_kernel_does_not_take():
    p = torch.nn.Parameter(torch.zeros(4, 4, device=DEV, dtype=torch.float64))
    p.grad = torch.zeros_like(p)
    with pytest.raises(RuntimeError, match="float32"):
        pkg.FusedAdam([p]).step()
    q = torch.nn.Parameter(torch.zeros(4, 4, device=DEV).t())
    q.grad = torch.zeros(4, 4, device=DEV)
    with pytest.raises(RuntimeError, match="contiguous"):
        pkg.FusedAdam([q]).step()


def test_state_dicts_interchange_with_torch_adam():
    lr, wd = 1e-3, 1e-5
    p0, gs = ref.adam_inputs(5003, seed=21)
    g = [torch.from_numpy(x).to(DEV) for x in gs]

    def run(kinds):
        p = torch.nn.Parameter(torch.from_numpy(p0).to(DEV))
        opt = kinds[0]([p], lr=lr, weight_decay=wd)
        for t in range(3):
            if t == 2 and kinds[1] is not kinds[0]:
                new = kinds[1]([p], lr=lr, weight_decay=wd)
                new.load_state_dict(opt.state_dict())
                opt = new
            p.grad = g[t]
            opt.step()
        return _np(p), _np(opt.state[p]["exp_avg"]), _np(opt.state[p]["exp_avg_sq"])

    def plain(params, **kw):
        return torch.optim.Adam(params, foreach=False, **kw)
    p64, m64, v64 = p0.astype(np.float64), np.zeros(5003), np.zeros(5003)
    gmax = 0.0
    for t in range(3):
        p64, m64, v64, g1 = ref.adam_step(p64, gs[t], m64, v64, lr, 0.9, 0.999, 1e-8, wd, t + 1)
        gmax = max(gmax, float(np.abs(g1).max()))
    torchs = run((plain, plain))
    for tag, kinds in (("fused,fused,torch", (pkg.FusedAdam, plain)), ("torch,torch,fused", (plain, pkg.FusedAdam)), ("fused x3", (pkg.FusedAdam, pkg.FusedAdam))):
        _adam_rule(tag, run(kinds), torchs, (p64, m64, v64, gmax), lr)


def test_scheduler_lr_reaches_the_kernel():
    """g = 0, wd = 0, eps = 1, m of known size: one step moves p by exactly lr / (1 - beta1) * beta1 m; a halved lr halves it."""
    def delta(opt, p):
        p.grad = torch.zeros_like(p)
        opt.state[p]["step"] = torch.tensor(0.0)
        opt.state[p]["exp_avg"] = torch.full_like(p, 0.5)
        opt.state[p]["exp_avg_sq"] = torch.zeros_like(p)
        before = p.detach().clone()
        opt.step()
        return before - p.detach()
    p = torch.nn.Parameter(torch.zeros(9, device=DEV))            # p = -delta exactly: no rounding against a larger p
    opt = pkg.FusedAdam([p], lr=2.0 ** -10, eps=1.0, weight_decay=0.0)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="max", factor=0.5, patience=0)
    d1 = delta(opt, p)
    sched.step(50.0)
    sched.step(50.0)                                               # no improvement: the plateau scheduler halves the group's lr
    assert opt.param_groups[0]["lr"] == 2.0 ** -11
    d2 = delta(opt, p)
    assert torch.all(d1 > 0) and torch.equal(d2, d1 / 2)          # lr is a power of two: halving it is exact through every product
    assert abs(float(d1[0]) - 2.0 ** -10 / 0.1 * 0.45) <= 2 ** -20 * float(d1[0])


# ======================================================================================================================================
# gradient norm
# ======================================================================================================================================
def test_grad_norm_and_clip_scale():
    v = _Views(seed=80, share_last_g=False)
    v.set_grads(0)
    grads = v.views(1)
    n64, _ = ref.clip([v.gs[k][0] for k in range(16)], 1.0)
    for max_norm in (1.0, n64 * 0.5, n64 * 4.0, float("inf")):
        norm, scale = ops.grad_norm(grads, max_norm)
        _, s64 = ref.clip([v.gs[k][0] for k in range(16)], max_norm)
        assert norm.dtype == torch.float64 and abs(float(norm) - n64) <= 2.0 ** -22 * n64
        if s64 == 1.0:
            assert float(scale) == 1.0                              # clip inactive
        else:                                                       # the norm's 2^-22 and one float32 rounding
            assert float(scale) < 1.0 and abs(float(scale) - s64) <= (2.0 ** -22 + U) * s64
    norm2, scale2 = ops.grad_norm(grads, 1.0)
    norm1, scale1 = ops.grad_norm(grads, 1.0)
    assert torch.equal(norm1, norm2) and torch.equal(scale1, scale2)          # bit-equal from run to run
    # the order is in element coordinates: contiguous, 16-byte aligned copies give the same bits as the views off the grid
    norm3, _ = ops.grad_norm([g.clone() for g in grads], 1.0)
    assert torch.equal(norm3, norm1)


# ======================================================================================================================================
# trainer
# ======================================================================================================================================
B = 16
MODELS = {"simple": pkg.SimpleWakewordModel, "full": pkg.WakewordModel}


def _batch(n, T, seed):
    g = torch.Generator().manual_seed(seed)
    x = (-40.0 + 20.0 * torch.randn(n, 1, 80, T, generator=g)).to(DEV)            # log-mel dB magnitudes
    y = torch.randint(0, 2, (n, 1), generator=g).to(DEV)
    return x, y


def _model(name, seed=1234):
    torch.manual_seed(seed)
    return MODELS[name]().to(DEV)


def _all_errors(named_ours, named_torch, f64, lr):
    keys = list(f64["p"])
    cat = lambda d: np.concatenate([np.asarray(d[k], np.float64).reshape(-1) for k in keys])      # noqa: E731
    ours = (cat(named_ours["p"]), cat(named_ours["m"]), cat(named_ours["v"]))
    torchs = (cat(named_torch["p"]), cat(named_torch["m"]), cat(named_torch["v"]))
    return ours, torchs, (cat(f64["p"]), cat(f64["m"]), cat(f64["v"]), f64["gmax"])


def _state_of(model, opt):
    named = dict(model.named_parameters())
    return {"p": {k: _np(p) for k, p in named.items()}, "m": {k: _np(opt.state[p]["exp_avg"]) for k, p in named.items()},
            "v": {k: _np(opt.state[p]["exp_avg_sq"]) for k, p in named.items()}}


def _f64_update(f64, grads, lr, wd, step, scale=1.0):
    for k in f64["p"]:
        f64["p"][k], f64["m"][k], f64["v"][k], g1 = ref.adam_step(f64["p"][k], grads[k], f64["m"][k], f64["v"][k], lr, 0.9, 0.999, 1e-8, wd, step, scale)
        f64["gmax"] = max(f64["gmax"], float(np.abs(g1).max()))


@pytest.mark.parametrize("name, T", [("simple", 8), ("full", 8), ("simple", 32)])
def test_trainer_step_grads_update_and_first_batch(name, T):
    lr, wd = pkg.TrainingConfig.LEARNING_RATE, 1e-5
    model, twin = _model(name), _model(name)
    x, y = _batch(B, T, seed=3)
    trainer = pkg.WakewordTrainer(model, DEV)
    model.train(); twin.train()
    before = {k: _np(p).astype(np.float64) for k, p in model.named_parameters()}
    f64 = {"p": dict(before), "m": {k: np.zeros_like(v) for k, v in before.items()}, "v": {k: np.zeros_like(v) for k, v in before.items()}, "gmax": 0.0}
    torch.manual_seed(77)
    trainer.step(x, y)
    # ---- the hand loop's first batch on the twin, same seed: bit-equal logits, so the same correct count; the loss within the rule ----
    torch.manual_seed(77)
    out = twin(x)
    assert torch.equal(trainer.last_logits[:B], out.detach())
    hand_loss = F.cross_entropy(out.detach(), y.squeeze())
    l64 = ref.ce(_np(out), _np(y)[:, 0])[0]
    _rule("first-batch loss", abs(float(trainer.last_loss) - l64) / abs(l64), abs(float(hand_loss) - l64) / abs(l64), ref.CAP_LOSS)
    s = ops.read_loss_stats(trainer.train_stats)
    assert s["correct"] == int((torch.max(out.detach(), 1)[1] == y.squeeze()).sum()) and s["total"] == B and s["batches"] == 1
    # ---- gradients: bit-equal to autograd's through the same kernels, fed the same d loss / d logits ----
    out.backward(gradient=ops.ce_loss(out.detach(), y)[1])
    tnamed, named = dict(twin.named_parameters()), dict(model.named_parameters())
    for k, p in named.items():
        assert torch.equal(p.grad, tnamed[k].grad), k
    assert named["lstm.bias_hh_l0"].grad is named["lstm.bias_ih_l0"].grad and named["lstm.bias_hh_l1"].grad is named["lstm.bias_ih_l1"].grad
    assert not named["lstm.weight_hh_l0"].grad.any() and not named["lstm.weight_hh_l1"].grad.any()
    # ---- the update: torch's Adam on the twin fed those gradients is the reference, the float64 restatement the truth ----
    topt = torch.optim.Adam(twin.parameters(), lr=lr, weight_decay=wd, foreach=False)
    topt.step()
    _f64_update(f64, {k: _np(p.grad) for k, p in named.items()}, lr, wd, 1)
    o, tt, f = _all_errors(_state_of(model, trainer.optimizer), _state_of(twin, topt), f64, lr)
    _adam_rule(f"{name} T={T} step 1", o, tt, f, lr)
    for k in ("lstm.weight_hh_l0", "lstm.weight_hh_l1"):           # moved, by weight decay alone: g' = wd p
        moved = _np(named[k]).astype(np.float64) - before[k]
        assert np.all(moved[before[k] != 0] != 0) and np.all(np.sign(moved) == -np.sign(before[k]))
        assert np.max(np.abs(moved)) <= lr * (1 + 1e-3)
    if T != 8 or name != "simple":
        return
    # ---- three further steps, each fed the trainer's own gradients ----
    for t in range(2, 5):
        xb, yb = _batch(B, T, seed=10 + t)
        trainer.step(xb, yb)
        for k, p in named.items():
            tnamed[k].grad = p.grad.clone()
        topt.step()
        _f64_update(f64, {k: _np(p.grad) for k, p in named.items()}, lr, wd, t)
        o, tt, f = _all_errors(_state_of(model, trainer.optimizer), _state_of(twin, topt), f64, lr)
        _adam_rule(f"{name} step {t}", o, tt, f, lr)


def test_trainer_step_full_model_three_further_steps():
    lr, wd = pkg.TrainingConfig.LEARNING_RATE, 1e-5
    model, twin = _model("full"), _model("full")
    trainer = pkg.WakewordTrainer(model, DEV)
    model.train()
    named, tnamed = dict(model.named_parameters()), dict(twin.named_parameters())
    before = {k: _np(p).astype(np.float64) for k, p in named.items()}
    f64 = {"p": dict(before), "m": {k: np.zeros_like(v) for k, v in before.items()}, "v": {k: np.zeros_like(v) for k, v in before.items()}, "gmax": 0.0}
    topt = torch.optim.Adam(twin.parameters(), lr=lr, weight_decay=wd, foreach=False)
    torch.manual_seed(5)
    for t in range(1, 5):
        xb, yb = _batch(B, 8, seed=20 + t)
        trainer.step(xb, yb)
        for k, p in named.items():
            tnamed[k].grad = p.grad.clone()
        topt.step()
        _f64_update(f64, {k: _np(p.grad) for k, p in named.items()}, lr, wd, t)
        o, tt, f = _all_errors(_state_of(model, trainer.optimizer), _state_of(twin, topt), f64, lr)
        _adam_rule(f"full step {t}", o, tt, f, lr)


@pytest.mark.parametrize("name", ["simple", "full"])
def test_epoch_bookkeeping_and_validate(name):
    model = _model(name)
    trainer = pkg.WakewordTrainer(model, DEV)
    x, y = _batch(37, 8, seed=8)
    batches = [(x[i:i + 16], y[i:i + 16]) for i in range(0, 37, 16)]                 # 16, 16 and a ragged 5
    seen = []

    def loader():
        for b in batches:
            yield b
            seen.append(float(trainer.last_loss))
    torch.manual_seed(1)
    loss, acc = trainer.train_epoch(loader())
    s = ops.read_loss_stats(trainer.train_stats)
    assert (s["total"], s["batches"]) == (37, 3) and len(seen) == 3
    assert s["loss_sum"] == seen[0] + seen[1] + seen[2] and loss == s["loss_sum"] / 3 and acc == 100.0 * s["correct"] / 37
    assert model.training                                           # train_epoch leaves train mode on, as the reference does
    # validate against the eval-mode hand loop
    vloss, vacc = trainer.validate(batches)
    assert not model.training
    hand, h64, correct = 0.0, 0.0, 0
    with torch.no_grad():
        for xb, yb in batches:
            out = model(xb)
            hand += F.cross_entropy(out, yb.squeeze(1)).item()
            h64 += ref.ce(_np(out), _np(yb)[:, 0])[0]
            correct += (torch.max(out, 1)[1] == yb.squeeze(1)).sum().item()
    assert vacc == 100.0 * correct / 37
    _rule("validate loss", abs(vloss - h64 / 3) / (h64 / 3), abs(hand / 3 - h64 / 3) / (h64 / 3), ref.CAP_LOSS)
    # a label outside {0, 1} is an error at the end of the epoch; targets of [B] are taken as well as [B, 1]
    trainer.validate([(x[:4], y[:4, 0])])
    bad = y[:4].clone()
    bad[2] = 2
    with pytest.raises(ValueError, match="labels"):
        trainer.validate([(x[:4], bad)])
    with pytest.raises(ValueError, match="labels"):
        trainer.train_epoch([(x[:4], bad)])


def test_train_schedules_stops_early_and_saves_the_reference_checkpoint(tmp_path, capsys):
    model = _model("simple")
    path = str(tmp_path / "best.pth")
    trainer = pkg.WakewordTrainer(model, DEV, checkpoint_path=path)
    assert trainer.patience == 10 and trainer.scheduler.patience == 5 and trainer.scheduler.factor == 0.5 and trainer.scheduler.mode == "max"
    assert isinstance(trainer.optimizer, pkg.FusedAdam) and trainer.optimizer.defaults["weight_decay"] == 1e-5
    assert trainer.optimizer.defaults["lr"] == pkg.TrainingConfig.LEARNING_RATE and isinstance(trainer.criterion, torch.nn.CrossEntropyLoss)
    trainer.scheduler.patience = 0
    trainer.patience = 1
    x, y = _batch(16, 8, seed=2)
    # validation: one clip 8 times with labels 0, 1, 0, 1, ...: the accuracy is 50 % whatever the model predicts, so epoch 2 cannot improve
    xv = x[:1].repeat(8, 1, 1, 1)
    yv = torch.tensor([0, 1] * 4, device=DEV).view(8, 1)
    torch.manual_seed(0)
    best = trainer.train([(x, y)], [(xv, yv)], epochs=5)
    assert best == 50.0 == trainer.best_val_acc and trainer.epochs_no_improve == 1
    assert len(trainer.train_losses) == len(trainer.val_losses) == len(trainer.train_accuracies) == len(trainer.val_accuracies) == 2
    assert trainer.optimizer.param_groups[0]["lr"] == pkg.TrainingConfig.LEARNING_RATE / 2          # halved after the non-improving epoch
    text = capsys.readouterr().out
    assert "Early stopping triggered! No improvement for 1 epochs." in text and "Total epochs trained: 2" in text
    assert "New best model saved! Validation accuracy: 50.00%" in text and text.isascii()
    ckpt = torch.load(path, weights_only=True)
    assert sorted(ckpt) == sorted(["epoch", "model_state_dict", "optimizer_state_dict", "val_acc", "train_acc", "train_loss", "val_loss"])
    assert ckpt["epoch"] == 0 and ckpt["val_acc"] == 50.0
    fresh = pkg.SimpleWakewordModel().to(DEV)
    from wakeword_jupyterlab_amd.model import load_checkpoint
    load_checkpoint(fresh, path)
    topt = torch.optim.Adam(fresh.parameters())
    topt.load_state_dict(ckpt["optimizer_state_dict"])
    assert float(topt.state[fresh.fc.weight]["step"]) == 1.0
    fopt = pkg.FusedAdam(fresh.parameters())
    fopt.load_state_dict(ckpt["optimizer_state_dict"])
    # the checkpoint holds the weights of epoch 1, the model those of epoch 2: the eval forward sees the newer ones (packed weights follow)
    model.eval(); fresh.eval()
    with torch.no_grad():
        assert not torch.equal(model(xv), fresh(xv))


def test_step_has_no_hidden_waits_and_allocates_nothing():
    model = _model("simple")
    trainer = pkg.WakewordTrainer(model, DEV)
    model.train()
    x, y = _batch(B, 8, seed=6)
    y = y.contiguous()
    for _ in range(2):
        trainer.step(x, y)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        trainer.step(x, y)
        trainer.step(x, y)
        before = torch.cuda.memory_allocated()
        trainer.step(x, y)
        after = torch.cuda.memory_allocated()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert before == after
    torch.cuda.synchronize()
    assert ops.read_loss_stats(trainer.train_stats)["batches"] == 5


@pytest.mark.parametrize("name", ["simple", "full"])
def test_max_grad_norm_clips_after_the_backward(name):
    lr, wd = pkg.TrainingConfig.LEARNING_RATE, 1e-5
    model, twin = _model(name), _model(name)
    with torch.no_grad():                                           # a head that has grown, as after some training: a fresh model's gradient
        model.fc.weight.mul_(20.0)                                  # norm is about 0.4 and would leave the clip idle
        twin.fc.weight.mul_(20.0)
    trainer = pkg.WakewordTrainer(model, DEV, max_grad_norm=1.0)
    model.train()
    named, tnamed = dict(model.named_parameters()), dict(twin.named_parameters())
    before = {k: _np(p).astype(np.float64) for k, p in named.items()}
    f64 = {"p": dict(before), "m": {k: np.zeros_like(v) for k, v in before.items()}, "v": {k: np.zeros_like(v) for k, v in before.items()}, "gmax": 0.0}
    x, y = _batch(B, 8, seed=12)
    torch.manual_seed(3)
    trainer.step(x, y)
    grads = {k: _np(p.grad) for k, p in named.items()}              # the kernel scales inside: the buffers keep the unclipped gradients
    n64, s64 = ref.clip(list(grads.values()), 1.0)
    print(f"{name}: gradient norm {n64:.4f}, scale {s64:.6f}")
    assert s64 < 1.0, "the batch does not exercise the clip"
    assert abs(float(trainer._norm) - n64) <= 2.0 ** -22 * n64 and abs(float(trainer._scale) - s64) <= (2.0 ** -22 + U) * s64
    for k, p in named.items():
        tnamed[k].grad = p.grad.clone()
    torch.nn.utils.clip_grad_norm_(twin.parameters(), max_norm=1.0)
    topt = torch.optim.Adam(twin.parameters(), lr=lr, weight_decay=wd, foreach=False)
    topt.step()
    _f64_update(f64, grads, lr, wd, 1, scale=s64)
    o, tt, f = _all_errors(_state_of(model, trainer.optimizer), _state_of(twin, topt), f64, lr)
    _adam_rule(f"{name} clipped", o, tt, f, lr)
