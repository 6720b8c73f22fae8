"""Knowledge distillation on the GPU (distill_loss_kernel in csrc/ww_optim.hip): the kernel against the float64
restatement of tests/distill_ref.py, its structure (alpha = 0, repeats, non-finite teacher rows, empty terms), and WakewordTrainer's
step with a teacher against a hand-written loop over the same native calls.

Bounds (distill_ref): |loss - ref| <= 2^-23 |ref| + 1e-12 and |d - ref| <= 2^-23 |ref| + 1e-12 * (alpha T + (1 - alpha) max(w, 1)) /
denominator, each part of the absolute term over its own term's denominator -- one float32 rounding of a float64 result, plus the
cancellation in p - q.  Integer statistics are equal exactly; everything the trainer does is compared bit for bit."""
import gc

import numpy as np
import pytest
import torch
import torch.nn as nn

import distill_ref as ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import ops, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GUARD = -77.25


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _offset(a):
    """`a` on the device one row past the start of a 16-byte aligned buffer: off the 16-byte grid (a row is 8 bytes), guard values around it."""
    a = np.ascontiguousarray(a)
    buf = torch.full((a.shape[0] + 2,) + a.shape[1:], GUARD if a.dtype.kind == "f" else -7, dtype=torch.from_numpy(a).dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + a.shape[0]]
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 8
    return buf, view


# ======================================================================================================================================
# the kernel against float64
# ======================================================================================================================================
@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("n", ref.SIZES)
def test_kernel_matches_the_float64_restatement(n, shifted):
    z, zt, y, t = ref.inputs(n)
    if shifted:
        (_, zd), (_, ztd), (_, yd), (_, td) = _offset(z), _offset(zt), _offset(y), _offset(t)
        dbuf = torch.full((n + 2, 2), GUARD, device=DEV)
        d = dbuf[1:n + 1]
    else:
        zd, ztd, yd, td = _dev(z), _dev(zt), _dev(y), _dev(t)
        dbuf = torch.full((n + 2, 2), GUARD, device=DEV)                 # [n + 2, 2] float32 from the caching allocator: 16-byte aligned
        d = dbuf[:n]
        assert all(x.data_ptr() % 16 == 0 for x in (zd, ztd, yd, td, d))
    loss = torch.zeros((), device=DEV)
    worst_loss, worst_d = -np.inf, -np.inf
    for tag, kind, opts, alpha, T in ref.grid():
        target = ref.target_of(kind, y, t)
        want = ref.distill(z, zt, target, alpha, T, **opts)
        stats, dstats = ops.new_loss_stats(DEV), ops.new_distill_stats(DEV)
        dbuf.fill_(GUARD)
        ops.distill_loss_into(zd, ztd, ref.target_of(kind, yd, td), d, loss, stats, dstats, alpha=alpha, temperature=T, **opts)
        got, gd = float(loss), _np(d).astype(np.float64)
        e_loss, e_d = ref.loss_excess(got, want["loss"]), ref.dlogits_excess(gd, want)
        worst_loss, worst_d = max(worst_loss, e_loss), max(worst_d, e_d)
        assert e_loss <= 0.0, f"{tag} n={n}: loss {got!r} against {want['loss']!r}"
        assert e_d <= 0.0, f"{tag} n={n}: a gradient element misses its bound by {e_d:.3e}"
        outside = torch.cat([dbuf[:1], dbuf[n + 1:]]) if shifted else dbuf[n:]
        assert torch.all(outside == GUARD), f"{tag} n={n}: the kernel wrote outside dlogits"
        s, ds = ops.read_loss_stats(stats), ops.read_distill_stats(dstats)
        assert {k: s[k] for k in want["stats"]} == want["stats"] and s["batches"] == 1, tag
        assert {k: ds[k] for k in want["dstats"]} == want["dstats"] and ds["batches"] == 1, tag
        assert s["loss_sum"] == got or (got != got and s["loss_sum"] != s["loss_sum"]), tag
        for key in ("hard", "kd"):
            assert abs(ds[key + "_sum"] - want[key]) <= ref.loss_bound(want[key]), f"{tag} n={n}: {key}_sum {ds[key + '_sum']!r} against {want[key]!r}"
    print(f"n={n} {'offset' if shifted else 'aligned'}: largest (error - bound): loss {worst_loss:.3e}, dlogits {worst_d:.3e}")


# ======================================================================================================================================
# structure
# ======================================================================================================================================
@pytest.mark.parametrize("n", (3, 257, 1025))
def test_alpha_zero_has_the_bits_of_the_hard_loss_alone(n):
    z, zt, y, t = ref.inputs(n)
    zd, ztd, yd, td = _dev(z), _dev(zt), _dev(y), _dev(t)
    clean = _dev(np.where((y == 0) | (y == 1), y, 0))                               # the plain kernel's rule: no -100, no label 7
    cases = [(clean, ops.ce_loss, {}), (clean, ops.ce_loss, {"reduction": "sum"})]
    cases += [(yd, ops.ce_loss, o) for _, k, o in ref.OPTION_SETS if k == "labels" and o]
    cases += [(td, ops.soft_ce_loss, o) for _, k, o in ref.OPTION_SETS if k == "probs"]
    for target, plain, opts in cases:
        s_plain, s_kd = ops.new_loss_stats(DEV), ops.new_loss_stats(DEV)
        loss0, d0 = plain(zd, target, s_plain, **opts)
        for T in (0.05, 2.0):
            s_kd.zero_()
            loss1, d1 = ops.distill_loss(zd, ztd, target, s_kd, alpha=0.0, temperature=T, **opts)
            assert torch.equal(loss0, loss1) and torch.equal(d0, d1), (opts, T)
            assert torch.equal(s_plain, s_kd), (opts, T)


def test_two_runs_give_equal_bits():
    z, zt, y, t = ref.inputs(1025)
    zd, ztd, yd = _dev(z), _dev(zt), _dev(y)
    runs = []
    for _ in range(2):
        stats, dstats = ops.new_loss_stats(DEV), ops.new_distill_stats(DEV)
        loss, d = ops.distill_loss(zd, ztd, yd, stats, dstats, alpha=0.3, temperature=2.0, weight=(0.25, 4.0), label_smoothing=0.125)
        runs.append((loss.view(torch.int32).clone(), d.view(torch.int32).clone(), stats, dstats))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_non_finite_teacher_rows_are_counted_and_add_nothing():
    n = 257
    z, zt, y, t = ref.inputs(n, nonfinite_teacher=False)
    bad = zt.copy()
    rows = [0, 1, 100, 255, 256]
    bad[rows] = [(np.nan, 0.0), (np.inf, 1.0), (0.0, -np.inf), (np.nan, np.nan), (np.inf, np.inf)]
    keep = np.ones(n, bool)
    keep[rows] = False
    for target in (None, _dev(y)):
        dstats = ops.new_distill_stats(DEV)
        loss, d = ops.distill_loss(_dev(z), _dev(bad), target, None, dstats, alpha=1.0 if target is None else 0.3, temperature=2.0, reduction="sum")
        ds = ops.read_distill_stats(dstats)
        assert ds["teacher_nonfinite"] == len(rows) and ds["kd_rows"] == n - len(rows)
        assert np.isfinite(float(loss)) and bool(torch.isfinite(d).all())
        # the KD term of the remaining rows alone, under the sum (a mean would divide by another count): the same bits but for the order of
        # the float64 sum, so the bound of one rounding
        dstats2 = ops.new_distill_stats(DEV)
        ops.distill_loss(_dev(z[keep]), _dev(zt[keep]), None, None, dstats2, temperature=2.0, reduction="sum")
        kd, kd2 = ds["kd_sum"], ops.read_distill_stats(dstats2)["kd_sum"]
        assert abs(kd - kd2) <= ref.loss_bound(kd2)
        if target is None:
            assert torch.all(d[rows] == 0.0)                                        # no hard term: such a row moves nothing


def test_all_labels_ignored_leaves_the_teacher_term_alone():
    n = 65
    z, zt, _, _ = ref.inputs(n)
    zd, ztd = _dev(z), _dev(zt)
    ignored = torch.full((n,), -100, dtype=torch.int64, device=DEV)
    for alpha in (0.3, 1.0):
        dstats = ops.new_distill_stats(DEV)
        loss, d = ops.distill_loss(zd, ztd, ignored, None, dstats, alpha=alpha, temperature=2.0)
        want = ref.distill(z, zt, np.full(n, -100), alpha, 2.0)
        alone = ref.distill(z, zt, None, 1.0, 2.0)
        assert np.isfinite(float(loss)) and ref.loss_excess(float(loss), want["loss"]) <= 0.0
        assert abs(want["loss"] - alpha * alone["loss"]) <= 1e-15 * abs(want["loss"])       # the restatement itself: alpha x the KD part
        assert ref.dlogits_excess(_np(d), want) <= 0.0
        assert ops.read_distill_stats(dstats)["hard_rows"] == 0


def test_nothing_counted_gives_nan_and_a_zero_gradient():
    n = 65
    z, _, _, _ = ref.inputs(n)
    zd = _dev(z)
    nans = torch.full((n, 2), float("nan"), device=DEV)
    ignored = torch.full((n,), -100, dtype=torch.int64, device=DEV)
    for target, alpha in ((ignored, 0.3), (ignored, 0.0), (ignored, 1.0), (None, 0.5), (nans, 0.3)):
        stats, dstats = ops.new_loss_stats(DEV), ops.new_distill_stats(DEV)
        loss, d = ops.distill_loss(zd, nans, target, stats, dstats, alpha=alpha, temperature=2.0)
        assert float(loss) != float(loss)
        assert torch.equal(d.view(torch.int32), torch.zeros_like(d).view(torch.int32))      # exact zeros: not -0, not NaN
        ds = ops.read_distill_stats(dstats)
        assert ds["hard_sum"] == 0.0 and ds["kd_sum"] == 0.0 and ds["teacher_nonfinite"] == n and ds["batches"] == 1
    # under the sum nothing divides: the batch sums to 0, as ops.ce_loss does
    loss, d = ops.distill_loss(zd, nans, ignored, alpha=0.3, temperature=2.0, reduction="sum")
    assert float(loss) == 0.0 and not d.any()


def test_refusals_come_before_any_launch():
    z, zt, y, t = (_dev(a) for a in ref.inputs(8))
    d = torch.full((8, 2), GUARD, device=DEV)
    for kw in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(temperature=0.0), dict(temperature=-1.0),
               dict(temperature=float("inf")), dict(weight=(-1.0, 1.0)), dict(reduction="max")):
        with pytest.raises(ValueError):
            ops.distill_loss_into(z, zt, y, d, None, None, None, **kw)
    with pytest.raises(NotImplementedError):
        ops.distill_loss(z, zt, t, focal_gamma=2.0)
    with pytest.raises(ValueError):
        ops.distill_loss(z, zt, t, ignore_index=1)
    with pytest.raises((ValueError, TypeError)):
        ops.distill_loss(z, zt[:4], y)
    with pytest.raises(TypeError):
        ops.distill_loss(z, zt.double(), y)
    L = pkg._native.lib
    assert L.ww_distill_loss_f32(z.data_ptr(), None, y.data_ptr(), 0, 8, None, 0.5, 2.0, d.data_ptr(), None, None, None, None) != 0
    assert b"teacher" in L.ww_last_error()
    assert L.ww_distill_loss_f32(z.data_ptr(), zt.data_ptr(), y.data_ptr(), 2, 8, None, 0.5, 2.0, d.data_ptr(), None, None, None, None) != 0
    assert b"target_kind" in L.ww_last_error()
    torch.cuda.synchronize()
    assert torch.all(d == GUARD)


# ======================================================================================================================================
# trainer
# ======================================================================================================================================
MODELS = {"simple": pkg.SimpleWakewordModel, "full": pkg.WakewordModel}
OTHER = {"simple": "full", "full": "simple"}
SHAPES = ((3, 8), (16, 32))


def _batch(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    x = (-40.0 + 20.0 * torch.randn(B, 1, 80, T, generator=g)).to(DEV)
    y = torch.randint(0, 2, (B,), generator=g).to(DEV)
    return x, y


def _model(name, seed=1234, dropout=None):
    torch.manual_seed(seed)
    m = MODELS[name]().to(DEV)
    if dropout is not None:
        m.lstm.dropout = dropout
        m.dropout.p = dropout
    return m


def _pair(name, seed=1234):
    """(student, its identically seeded twin, a teacher of the OTHER class in eval mode); dropout 0 where bits are compared."""
    return _model(name, seed, 0.0).train(), _model(name, seed, 0.0).train(), _model(OTHER[name], seed + 1).eval()


class HandLoop:
    """The step written out over the public pieces: the teacher's eval forward, ops.train_forward_into, ops.distill_loss_into,
    ops.train_backward_into and FusedAdam with the trainer's settings."""

    def __init__(self, model):
        self.model, self.n_conv = model, model._n_conv
        keys = ops._train_keys(self.n_conv)
        named = dict(model.named_parameters())
        params = [named[k] for k in keys]
        self.grads = {k: torch.zeros_like(p) for k, p in zip(keys, params) if not k.startswith("lstm.bias_hh")}
        for k, p in zip(keys, params):
            p.grad = self.grads[k.replace("bias_hh", "bias_ih")]
        self.tp, self.tg = ops._train_params_struct(params, self.n_conv), ops.train_grads_struct(self.grads, self.n_conv)
        self.opt = pkg.FusedAdam(model.parameters(), lr=pkg.TrainingConfig.LEARNING_RATE, weight_decay=1e-5)
        self.loss = torch.zeros((), device=DEV)

    def step(self, x, zt, y, alpha, T, opts=None):
        B, m = x.shape[0], self.model
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        math = pkg._native.lib.ww_get_train_math()
        ws = torch.empty(ops.train_workspace_bytes(B, self.n_conv, math), device=DEV, dtype=torch.uint8)
        logits, dlogits = torch.empty((B, 2), device=DEV), torch.empty((B, 2), device=DEV)
        with torch.cuda.device(DEV):
            ops.train_forward_into(x, self.tp, m.lstm.dropout, m.dropout.p, seed, math, ws, logits)
            ops.distill_loss_into(logits, zt, y, dlogits, self.loss, None, None, alpha=alpha, temperature=T, opts=opts)
            ops.train_backward_into(x, self.tp, dlogits, math, ws, self.tg)
        self.opt.step()


def _same_training_state(trainer, other_model, other_opt):
    for (k, p), q in zip(trainer.model.named_parameters(), other_model.parameters()):
        assert torch.equal(p, q), k
        a, b = trainer.optimizer.state[p], other_opt.state[q]
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"]) and a["step"] == b["step"], k


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("name", ["simple", "full"])
def test_trainer_step_equals_the_hand_loop_bit_for_bit(name, B, T):
    model, twin, teacher = _pair(name)
    before = [p.detach().clone() for p in teacher.parameters()]
    trainer = pkg.WakewordTrainer(model, DEV, teacher=teacher, distill_alpha=0.3, distill_temperature=2.0)
    hand = HandLoop(twin)
    third = _model(name, 1234, 0.0).train()
    given = pkg.WakewordTrainer(third, DEV, teacher=teacher, distill_alpha=0.3, distill_temperature=2.0)      # fed teacher_logits=
    for k in range(3):
        x, y = _batch(B, T, seed=20 + k)
        with torch.no_grad():
            zt = teacher(x)
        trainer.step(x, y)
        assert torch.equal(trainer.last_teacher_logits, zt), k
        hand.step(x, zt, y, 0.3, 2.0)
        given.step(x, y, teacher_logits=zt)
        assert torch.equal(trainer.last_loss, hand.loss) and torch.equal(trainer.last_loss, given.last_loss), k
        assert bool(torch.isfinite(trainer.last_loss))
    _same_training_state(trainer, twin, hand.opt)
    _same_training_state(trainer, third, given.optimizer)
    assert torch.equal(trainer.distill_stats, given.distill_stats) and ops.read_distill_stats(trainer.distill_stats)["batches"] == 3
    for p, q in zip(teacher.parameters(), before):                                  # the teacher: not a bit moved, no gradient made
        assert torch.equal(p, q) and p.grad is None


@pytest.mark.parametrize("name", ["simple", "full"])
def test_trainer_steps_without_a_wait_or_an_allocation(name):
    model, _twin, teacher = _pair(name)
    trainer = pkg.WakewordTrainer(model, DEV, teacher=teacher)
    x, y = _batch(16, 32, seed=3)
    trainer.step(x, y)
    torch.cuda.synchronize()
    gc.collect()                                         # earlier tests' trainers (reference cycles) must not be freed inside the window
    torch.cuda.set_sync_debug_mode("error")
    try:
        before = torch.cuda.memory_allocated()
        for k in range(4):                                                          # steps 2..5
            trainer.step(x, y)
        after = torch.cuda.memory_allocated()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert before == after


def test_trainer_hard_term_on_mixup_targets_follows_the_probability_rule():
    import mixup_ref
    B, T = 16, 8
    model, twin, teacher = _pair("simple")
    crit = nn.CrossEntropyLoss(weight=torch.tensor((0.25, 4.0), device=DEV), label_smoothing=0.125)
    trainer = pkg.WakewordTrainer(model, DEV, criterion=crit, teacher=teacher, distill_alpha=0.3, distill_temperature=2.0)
    x, _ = _batch(B, T, seed=5)
    t = _dev(mixup_ref.soft_inputs(B, seed=77)[1])
    trainer.step(x, t)
    z, zt = trainer.last_logits[:B].clone(), trainer.last_teacher_logits.clone()
    want = ref.distill(_np(z), _np(zt), _np(t), 0.3, 2.0, weight=(0.25, 4.0), label_smoothing=0.125)
    assert ref.loss_excess(float(trainer.last_loss), want["loss"]) <= 0.0
    assert ref.dlogits_excess(_np(trainer._dlogits[:B]), want) <= 0.0
    hard, _ = ops.soft_ce_loss(z, t, weight=(0.25, 4.0), label_smoothing=0.125)      # the Probs rule itself
    assert ops.read_distill_stats(trainer.distill_stats)["hard_sum"] == float(hard)
    with pytest.raises(NotImplementedError):                                         # as without a teacher
        focal = pkg.WakewordTrainer(twin, DEV, criterion=pkg.FocalLoss(2.0), teacher=teacher)
        focal.step(x, t)


@pytest.mark.parametrize("name", ["simple", "full"])
def test_unlabelled_step_runs_and_moves_the_weights(name):
    model, twin, teacher = _pair(name)
    trainer = pkg.WakewordTrainer(model, DEV, teacher=teacher, distill_temperature=2.0)
    hand = HandLoop(twin)
    x, _ = _batch(3, 8, seed=9)
    before = [p.detach().clone() for p in model.parameters()]
    trainer.step(x, None)
    with torch.no_grad():
        hand.step(x, teacher(x), None, 0.5, 2.0)
    assert any(not torch.equal(p, q) for p, q in zip(model.parameters(), before))
    _same_training_state(trainer, twin, hand.opt)
    s, ds = ops.read_loss_stats(trainer.train_stats), ops.read_distill_stats(trainer.distill_stats)
    assert (s["total"], s["batches"], s["correct"], s["bad_labels"]) == (3, 1, 0, 0) and ds["hard_rows"] == 0 and ds["kd_rows"] == 3
    plain = pkg.WakewordTrainer(_model(name).train(), DEV)
    with pytest.raises(TypeError, match="teacher"):
        plain.step(x, None)


def test_mean_teacher_follows_the_students_updates():
    model = _model("simple", dropout=0.0).train()
    average = pkg.WeightAverage(model, decay=0.5)
    trainer = pkg.WakewordTrainer(model, DEV, average=average, teacher=average.model, distill_alpha=0.5)
    x, y = _batch(16, 8, seed=11)
    seen = []
    for k in range(3):
        trainer.step(x, y)
        seen.append(trainer.last_teacher_logits.clone())
        with torch.no_grad():
            now = average.model(x)                       # the averaged weights AFTER step k: what step k + 1 must use
        if k:
            assert torch.equal(seen[k], expected), k
            assert not torch.equal(seen[k], seen[k - 1]), k
        expected = now
    assert all(p.grad is None for p in average.model.parameters())


def test_no_teacher_is_bit_for_bit_what_it_was():
    # built and stepped before any distillation object exists in this test
    first = _model("simple").train()
    a = pkg.WakewordTrainer(first, DEV)
    batches = [_batch(16, 8, seed=30 + k) for k in range(3)]
    losses = []
    for k, (x, y) in enumerate(batches):
        torch.manual_seed(90 + k)
        losses.append(a.step(x, y).clone())
    teacher = _model("full", 99).eval()
    pkg.WakewordTrainer(_model("simple", 5).train(), DEV, teacher=teacher).step(*batches[0])
    second = _model("simple").train()
    b = pkg.WakewordTrainer(second, DEV)
    for k, (x, y) in enumerate(batches):
        torch.manual_seed(90 + k)
        assert torch.equal(b.step(x, y), losses[k]), k
    _same_training_state(a, second, b.optimizer)
    assert torch.equal(a.train_stats, b.train_stats) and b.distill_stats is None and b.distill_report is None


def test_thirty_unlabelled_steps_bring_the_student_towards_the_teacher():
    clips = synth.make_clips(0, 16)
    x = ops.logmel(torch.from_numpy(clips).to(DEV), True)
    model, teacher = _model("simple", dropout=0.0).train(), _model("full", 77).eval()
    trainer = pkg.WakewordTrainer(model, DEV, teacher=teacher, distill_temperature=2.0)
    kd = []
    for _ in range(30):
        trainer.distill_stats.zero_()
        trainer.step(x, None)
        kd.append(trainer.distill_stats.clone())
    first, last = (ops.read_distill_stats(r)["kd_sum"] for r in (kd[0], kd[-1]))
    print(f"KD term: step 1 {first:.6f}, step 30 {last:.6f}")
    assert last < first


def test_train_epoch_publishes_the_distillation_report():
    model, _, teacher = _pair("simple")
    trainer = pkg.WakewordTrainer(model, DEV, teacher=teacher, distill_alpha=0.3)
    loader = [_batch(16, 8, seed=40 + k) for k in range(3)]
    trainer.train_epoch(loader)
    loss, acc = trainer.train_epoch(loader)                                          # the records start again with every epoch
    r = trainer.distill_report
    assert r["batches"] == 3 and r["kd_rows"] == 48 and r["hard_rows"] == 48 and r["teacher_nonfinite"] == 0
    assert 0.0 <= r["agreement"] <= 100.0 and 0.0 <= r["teacher_accuracy"] <= 100.0
    assert abs(loss - (0.7 * r["hard_loss"] + 0.3 * r["kd_loss"])) <= 1e-6 * max(1.0, abs(loss))
    with torch.no_grad():
        want = sum(int(((teacher(x)[:, 1] > teacher(x)[:, 0]).long() == y).sum()) for x, y in loader)
    assert r["teacher_accuracy"] == 100.0 * want / 48
