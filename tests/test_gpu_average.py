"""WeightAverage on the GPU (adam_avg_kernel and weight_average_kernel in csrc/ww_optim.hip): the fused and the
stand-alone kernel against torch.lerp and a float64 recursion, FusedAdam and WakewordTrainer with an average attached.

Tolerances (tests/average_ref.py): the reference is torch.lerp in float32 on the same device over the float32 snapshots the kernel
produced; its error against the float64 recursion stays under a fixed cap, ours under twice the reference's + 2^-24.
Shapes: the 16-tensor size and phase table of tests/test_gpu_trainer.py for the kernels; B = 16, T = 8 for the models."""
import numpy as np
import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

import average_ref as aref
import test_gpu_trainer as tt
import trainer_ref as ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import average, ops

pytestmark = pytest.mark.gpu
DEV = tt.DEV
U = ref.U
ADAM = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)
# the average's phase on the 16-byte grid, per tensor of tt.SIZES: equal to the shared phase of p, g, m, v (the 16-byte path) in tensors
# 0, 1, 3, 4, 6, 7, 9 and 14, different (the one-float path) in 2, 5, 8 -- 64 blocks --, 13 and 15; 10..12 have unequal phases anyway
AVG_PHASES = [0, 1, 1, 1, 3, 2, 0, 2, 2, 1, 0, 1, 0, 3, 1, 0]


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return _np(t).view(np.int32)


class _Views(tt._Views):
    """tt._Views (p, g, m, v cut from guarded buffers) with a fifth role: the averages, guarded the same way, NaN until written."""

    def __init__(self, seed):
        super().__init__(seed)
        self.avg_off, total = [], tt.GUARD
        for n, ph in zip(tt.SIZES, AVG_PHASES):
            start = -(-total // 4) * 4 + ph
            self.avg_off.append(start)
            total = start + n + tt.GUARD
        self.avg_buf = torch.full((total + 4,), tt.GUARD_VALUE, device=DEV)
        assert self.avg_buf.data_ptr() % 16 == 0
        for a in self.avgs():
            a.fill_(float("nan"))

    def avgs(self):
        return [self.avg_buf[o:o + n] for o, n in zip(self.avg_off, tt.SIZES)]

    def avg_cat(self):
        return torch.cat(self.avgs())

    def p_cat(self):
        return torch.cat(self.views(0))

    def guards_intact(self):
        mask = torch.ones_like(self.avg_buf, dtype=torch.bool)
        for o, n in zip(self.avg_off, tt.SIZES):
            mask[o:o + n] = False
        return super().guards_intact() and bool(torch.all(self.avg_buf[mask] == tt.GUARD_VALUE))

    def fused(self, t, w, grad_scale=None):
        ops.adam_average_step(self.views(0), self.views(1), self.views(2), self.views(3), self.avgs(), step=t + 1, avg_weight=w,
                              grad_scale=grad_scale, **ADAM)

    def plain(self, t, grad_scale=None):
        ops.adam_step(self.views(0), self.views(1), self.views(2), self.views(3), step=t + 1, grad_scale=grad_scale, **ADAM)

    def same_state(self, other):
        return all(np.array_equal(self.cat(r).view(np.int32), other.cat(r).view(np.int32)) for r in (0, 2, 3))


def _check_rule(name, ours, snaps, weights, cap):
    """`ours` and `snaps` are device tensors: the reference runs torch.lerp over the same snapshots there; float64 on the host."""
    a64 = aref.recursion([_np(s) for s in snaps], weights)
    pmax = max(float(np.abs(_np(s)).max()) for s in snaps)
    aref.rule(name, aref.error(_np(ours), a64, pmax), aref.error(_np(aref.lerp_reference(snaps, weights)), a64, pmax), cap)


# ======================================================================================================================================
# the two kernels
# ======================================================================================================================================
def test_fused_kernel_16_tensors_3_steps():
    v, twin = _Views(seed=40), tt._Views(seed=40)
    weights, snaps = [1.0, 0.1, 0.5], []
    for t, w in enumerate(weights):
        v.set_grads(t)
        twin.set_grads(t)
        v.fused(t, w)
        ops.adam_step(twin.views(0), twin.views(1), twin.views(2), twin.views(3), step=t + 1, **ADAM)
        snaps.append(v.p_cat().clone())
    assert v.guards_intact() and twin.guards_intact()
    assert all(np.array_equal(v.cat(r).view(np.int32), twin.cat(r).view(np.int32)) for r in (0, 2, 3))      # p, m, v: ww_adam_step_f32's bits
    _check_rule("fused, weights 1, 0.1, 0.5", v.avg_cat(), snaps, weights, aref.CAP_SHORT)


@pytest.mark.parametrize("scaled", [False, True])
def test_fused_equals_adam_then_stand_alone_average(scaled):
    st = torch.tensor([0.25], device=DEV) if scaled else None
    v, w2 = _Views(seed=60), _Views(seed=60)
    for t, w in enumerate([1.0, 0.1, 0.5]):
        v.set_grads(t)
        w2.set_grads(t)
        v.fused(t, w, st)
        w2.plain(t, st)
        ops.weight_average(w2.views(0), w2.avgs(), w)
        assert np.array_equal(_bits(v.avg_cat()), _bits(w2.avg_cat())), (t, w)
    assert v.same_state(w2) and v.guards_intact() and w2.guards_intact()
    assert not torch.isnan(v.avg_cat()).any()


def test_copy_and_no_op_weights():
    v, twin = _Views(seed=70), _Views(seed=70)
    v.set_grads(0)
    twin.set_grads(0)
    v.fused(0, 1.0)                                                # over a NaN-filled average: p's exact bits, the NaN never read
    twin.plain(0)
    assert np.array_equal(_bits(v.avg_cat()), _bits(v.p_cat())) and v.same_state(twin)
    alone = _Views(seed=70)
    ops.weight_average(alone.views(0), alone.avgs(), 1.0)          # the stand-alone kernel's copy
    assert np.array_equal(_bits(alone.avg_cat()), _bits(alone.p_cat())) and alone.guards_intact()
    # w = 0: the average keeps its bits -- NaNs with a payload and negative zeros included -- while p, m and v advance
    marks = torch.tensor([0x7FC01234, -0x003FEDCC, -0x80000000, 0x00000001], dtype=torch.int32, device=DEV).view(torch.float32)
    for a in v.avgs():
        a[:4] = marks[:a.numel()]
    before = _bits(v.avg_cat()).copy()
    v.set_grads(1)
    twin.set_grads(1)
    v.fused(1, 0.0)
    twin.plain(1)
    ops.weight_average(v.views(0), v.avgs(), 0.0)
    assert np.array_equal(_bits(v.avg_cat()), before) and v.same_state(twin) and v.guards_intact()
    assert not np.array_equal(_np(v.p_cat()), _np(alone.p_cat()))


@pytest.mark.parametrize("mode, decay, warmup", [("ema", 0.999, False), ("ema", 0.9, True), ("swa", 0.0, False)])
def test_fifty_stand_alone_updates(mode, decay, warmup):
    rng = np.random.default_rng(5)
    sizes = [5, 300, 4097]
    ps = [torch.from_numpy((0.1 * rng.standard_normal(n)).astype(np.float32)).to(DEV) for n in sizes]
    avgs = [torch.full_like(p, float("nan")) for p in ps]
    weights, snaps = [], []
    for n in range(50):
        for p in ps:                                               # a random walk, as a parameter under training
            p.add_(torch.from_numpy((1e-3 * rng.standard_normal(p.numel())).astype(np.float32)).to(DEV))
        weights.append(average.update_weight(n, mode, decay, warmup))
        ops.weight_average(ps, avgs, weights[-1])
        snaps.append(torch.cat(ps).clone())
    _check_rule(f"50 updates {mode} {decay} warmup={warmup}", torch.cat(avgs), snaps, weights, aref.CAP_50)


# ======================================================================================================================================
# FusedAdam
# ======================================================================================================================================
class _Bag(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        self.w = torch.nn.ParameterList(params)


def _count_launchers(monkeypatch, names=("adam_launch", "adam_average_launch", "weight_average_launch")):
    calls = []
    for name in names:
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda table, *a, _real=real, _name=name, **k: (calls.append((_name, len(table))), _real(table, *a, **k))[1])
    return calls


def test_fused_adam_with_an_average(monkeypatch):
    calls = _count_launchers(monkeypatch)
    many, twin = tt._params17(7), tt._params17(7)
    bag = _Bag([p for p, _ in many])
    opt = pkg.FusedAdam(bag.parameters(), lr=1e-3, weight_decay=1e-5)
    opt.average = wa = pkg.WeightAverage(bag, decay=0.9)
    plain = pkg.FusedAdam([p for p, _ in twin], lr=1e-3, weight_decay=1e-5)
    twin_avgs = [torch.full_like(p, float("nan")) for p, _ in twin]
    for t in range(3):
        for p, gs in many + twin:
            p.grad = gs[t]
        if t == 2:
            many[4][0].grad = twin[4][0].grad = None               # a parameter without a gradient: averaged on its own
        del calls[:]
        opt.step()
        want = [("adam_average_launch", 16), ("adam_average_launch", 1)] if t < 2 else [("adam_average_launch", 16), ("weight_average_launch", 1)]
        assert calls == want and wa.n_averaged == t + 1 == wa.n_calls
        plain.step()
        ops.weight_average([p for p, _ in twin], twin_avgs, average.update_weight(t, "ema", 0.9))
    for i, ((p, _), (q, _)) in enumerate(zip(many, twin)):
        assert torch.equal(p, q) and np.array_equal(_bits(wa.average_of(p)), _bits(twin_avgs[i]))
        assert wa.average_of(p)._version >= 3 and not wa.average_of(p).requires_grad
        if i != 4:
            assert torch.equal(opt.state[p]["exp_avg_sq"], plain.state[q]["exp_avg_sq"])
    # the average is no optimiser state: torch's keys, and the state dict loads into torch.optim.Adam
    sd = opt.state_dict()
    assert sorted(sd) == ["param_groups", "state"] and all(sorted(s) == ["exp_avg", "exp_avg_sq", "step"] for s in sd["state"].values())
    assert sorted(sd["param_groups"][0]) == sorted(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"][0])
    topt = torch.optim.Adam([p for p, _ in twin], lr=1e-3, weight_decay=1e-5)
    topt.load_state_dict(sd)
    assert float(topt.state[twin[0][0]]["step"]) == 3.0 and float(topt.state[twin[4][0]]["step"]) == 2.0
    # an every="epoch" average is not fused, and one that is still skipping leaves the plain launch alone
    for other in (pkg.WeightAverage(bag, every="epoch"), pkg.WeightAverage(bag, start=5)):
        opt.average = other
        many[4][0].grad = many[4][1][0]
        del calls[:]
        opt.step()
        assert [c[0] for c in calls] == ["adam_launch", "adam_launch"] and other.n_averaged == 0
        assert other.n_calls == (1 if other.every == "step" else 0)


# ======================================================================================================================================
# trainer
# ======================================================================================================================================
B, T = 16, 8


@pytest.mark.parametrize("name", ["simple", "full"])
def test_trainer_steps_against_a_device_side_averaged_model(name):
    d = 0.99
    model = tt._model(name)
    wa = pkg.WeightAverage(model, decay=d)
    trainer = pkg.WakewordTrainer(model, DEV, average=wa)
    am = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(d))            # torch's float32 foreach lerp on the same device
    model.train()
    torch.manual_seed(3)
    flat = lambda m: torch.cat([p.detach().reshape(-1) for p in m.parameters()])  # noqa: E731
    snaps = []
    for i in range(5):
        x, y = tt._batch(B, T, seed=20 + i)
        trainer.step(x, y)
        am.update_parameters(model)
        snaps.append(flat(model).clone())
    assert wa.n_averaged == 5 == int(am.n_averaged)
    a64 = aref.recursion([_np(s) for s in snaps], [average.update_weight(n, "ema", d) for n in range(5)])
    pmax = max(float(s.abs().max()) for s in snaps)
    aref.rule(f"trainer {name}, 5 steps", aref.error(_np(flat(wa.model)), a64, pmax), aref.error(_np(flat(am.module)), a64, pmax), aref.CAP_SHORT)
    assert not torch.equal(flat(wa.model), flat(model))


def test_average_changes_nothing_else_and_adds_no_launch(monkeypatch):
    names = ("train_forward_into", "ce_loss_into", "soft_ce_loss_into", "train_backward_into", "grad_norm_launch", "adam_launch",
             "adam_average_launch", "weight_average_launch")
    x, y = tt._batch(B, T, seed=6)
    y = y.contiguous()
    runs = {}
    for with_average in (False, True):
        model = tt._model("full")
        wa = pkg.WeightAverage(model) if with_average else None
        trainer = pkg.WakewordTrainer(model, DEV, average=wa)
        model.train()
        torch.manual_seed(11)
        for _ in range(2):
            trainer.step(x, y)
        torch.cuda.synchronize()
        calls = _count_launchers(monkeypatch, names)
        torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(2):
                trainer.step(x, y)
        finally:
            torch.cuda.set_sync_debug_mode("default")
            monkeypatch.undo()
        torch.cuda.synchronize()
        runs[with_average] = (tt._state_of(model, trainer.optimizer), [c[0] for c in calls], wa)
    (plain, plain_calls, _), (avgd, avg_calls, wa) = runs[False], runs[True]
    for role in "pmv":
        for k in plain[role]:
            assert np.array_equal(plain[role][k].view(np.int32), avgd[role][k].view(np.int32)), (role, k)
    assert len(plain_calls) == len(avg_calls) == 2 * 4
    assert [c.replace("adam_average_launch", "adam_launch") for c in avg_calls] == plain_calls
    assert avg_calls.count("adam_average_launch") == 2 and "weight_average_launch" not in avg_calls and wa.n_averaged == 4


def _validation_set():
    x, y = tt._batch(24, T, seed=31)
    return [(x[:16], y[:16]), (x[16:], y[16:])]


def test_evaluate_average_follows_the_averaged_model():
    model = tt._model("simple")
    with pytest.raises(ValueError, match="average"):
        pkg.WakewordTrainer(model, DEV, evaluate="average")
    with pytest.raises(ValueError, match="evaluate"):
        pkg.WakewordTrainer(model, DEV, evaluate="ema")
    with pytest.raises(ValueError, match="another model"):
        pkg.WakewordTrainer(model, DEV, average=pkg.WeightAverage(tt._model("simple")))
    wa = pkg.WeightAverage(model, decay=0.5)
    trainer = pkg.WakewordTrainer(model, DEV, average=wa, evaluate="average")
    val = _validation_set()
    torch.manual_seed(2)
    for round_ in range(2):                                        # the second round: a further update, so the packed weights were rebuilt
        model.train()
        for i in range(2):
            trainer.step(*tt._batch(B, T, seed=40 + 2 * round_ + i))
        got = trainer.validate(val)
        fresh = tt.MODELS["simple"]().to(DEV)
        fresh.load_state_dict(wa.model.state_dict())
        judge = pkg.WakewordTrainer(fresh, DEV)
        assert judge.validate(val) == got and judge.val_report == trainer.val_report
        assert not model.training and not wa.model.training
        raw = pkg.WakewordTrainer(model, DEV)
        assert raw.validate(val)[0] != got[0]                      # ... and it is not the raw weights' loss
    assert wa.n_averaged == 4


def test_checkpoint_keys_and_resuming(tmp_path):
    x, y = tt._batch(3 * B, T, seed=50)
    batches = [(x[i:i + B], y[i:i + B]) for i in range(0, 3 * B, B)]
    xv = x[:1].repeat(8, 1, 1, 1)
    yv = torch.tensor([0, 1] * 4, device=DEV).view(8, 1)           # 50 % whatever the model says: the first epoch is the best one
    seven = sorted(["epoch", "model_state_dict", "optimizer_state_dict", "val_acc", "train_acc", "train_loss", "val_loss"])

    def fresh(path, with_average=True):
        model = tt._model("simple")
        wa = pkg.WeightAverage(model, decay=0.9, warmup=True) if with_average else None
        return model, wa, pkg.WakewordTrainer(model, DEV, checkpoint_path=path, average=wa)

    def three_more(trainer, model, seed):
        model.train()
        torch.manual_seed(seed)
        for b in batches:
            trainer.step(*b)

    m0, _, t0 = fresh(str(tmp_path / "plain.pth"), with_average=False)
    torch.manual_seed(0)
    t0.train(batches[:1], [(xv, yv)], epochs=1)
    assert sorted(torch.load(str(tmp_path / "plain.pth"), weights_only=True)) == seven
    # 3 steps, saved, loaded into a new trainer and average, 3 more steps ...
    m1, wa1, t1 = fresh(str(tmp_path / "avg.pth"))
    torch.manual_seed(0)
    t1.train(batches, [(xv, yv)], epochs=1)
    ckpt = torch.load(str(tmp_path / "avg.pth"), weights_only=True)
    assert sorted(ckpt) == sorted(seven + ["average_state_dict"]) and ckpt["average_state_dict"]["n_averaged"] == 3
    m2, wa2, t2 = fresh(str(tmp_path / "unused.pth"))
    m2.load_state_dict(ckpt["model_state_dict"])
    t2.optimizer.load_state_dict(ckpt["optimizer_state_dict"])
    wa2.load_state_dict(ckpt["average_state_dict"])
    three_more(t2, m2, seed=1)
    # ... against 6 uninterrupted steps
    m3, wa3, t3 = fresh(str(tmp_path / "straight.pth"))
    torch.manual_seed(0)
    t3.train(batches, [(xv, yv)], epochs=1)
    three_more(t3, m3, seed=1)
    assert wa2.n_averaged == 6 == wa3.n_averaged
    for (k, a), b, p, q in zip(wa2.model.named_parameters(), wa3.model.parameters(), m2.parameters(), m3.parameters()):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(p), _bits(q)), k
    assert not torch.equal(wa2.model.fc.weight, m2.fc.weight)


def test_epoch_swa_is_the_mean_of_the_late_snapshots():
    model = tt._model("simple")
    wa = pkg.WeightAverage(model, mode="swa", every="epoch", start=1)
    trainer = pkg.WakewordTrainer(model, DEV, average=wa)
    assert trainer.optimizer.average is wa                         # attached, but an every="epoch" average is never fused
    flat = lambda m: torch.cat([p.detach().reshape(-1) for p in m.parameters()])  # noqa: E731
    torch.manual_seed(4)
    snaps = []
    for e in range(3):
        trainer.train_epoch([tt._batch(B, T, seed=60 + e)])
        snaps.append(flat(model).clone())
        assert (wa.n_calls, wa.n_averaged) == (e + 1, e)
    a64 = 0.5 * (_np(snaps[1]).astype(np.float64) + _np(snaps[2]).astype(np.float64))
    pmax = max(float(s.abs().max()) for s in snaps[1:])
    reference = aref.lerp_reference(snaps[1:], [1.0, 0.5])
    aref.rule("epoch SWA", aref.error(_np(flat(wa.model)), a64, pmax), aref.error(_np(reference), a64, pmax), aref.CAP_SHORT)
