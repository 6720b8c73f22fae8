"""WakewordTrainer.step with its options composed: QAT with a clipped quantiser, a fixed or a mean teacher,
class-probability targets, weighted / smoothed / focal losses, loss-ranked selection, the gradient-norm clip, the averaged weights in
the Adam launch and the ledger, several at a time, over batches that shrink and grow -- B = 19, 5, 19, 33 and once more 33.

Every step is checked as a chain of stage contracts, each on the stage's OWN input read back from the device (tests/step_ref.py composes
the float64 / numpy restatements every option already has): 1 the quantiser's output, 2 the scoring pass, the selection and the gather,
3 the train forward, 4 the teacher's forward, 5 loss, gradient and counters, 6 backward and straight-through mask, 7 norm and clip scale,
8 Adam and the average, 9 the ledger; then the launches of the step, in order, and -- on the second B = 19 step and the second B = 33
step -- no wait and no allocation.  One documented exception: a mean teacher's packed weights are rebuilt through the host after every
update, "a copy and a wait" (a new device tensor and a blocking copy per step), so the quiet-step check does
not apply to that configuration; its nine contracts and its launches are checked like everyone's.

Tolerances: none of this file's own.  Bit equality wherever the same kernels run on the same inputs (1, 2's logits and gather, 3, 4, 6,
8's stand-alone launch, 9); select_ref.bound for the scores; distill_ref.loss_bound / dlogits_bound beside a teacher, else the rule of
trainer_ref (`allowed`, under loss_ref's and mixup_ref's caps) over torch's float32 result; trainer_ref.norm_bound / scale_bound;
trainer_ref's CAP_P / CAP_M / CAP_V and average_ref.CAP_SHORT."""
import gc

import numpy as np
import pytest
import torch

import average_ref as aref
import distill_ref
import loss_ref
import mixup_ref
import step_ref as sr
import test_gpu_qat as tqat
import test_gpu_quant as tq
import test_gpu_trainer as tt
import trainer_ref as ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import ops
from wakeword_jupyterlab_amd.average import update_weight

pytestmark = pytest.mark.gpu
DEV = tt.DEV
_np, _bits_equal = tq._np, tq._bits_equal
MATHS = ("f16x3", "f32")                                         # the arithmetics tests/test_gpu_train.py parametrises (its train_math fixture)
SEED = 100                                                       # step i runs under torch.manual_seed(SEED + i)


def _criterion(opts):
    if opts is None:
        return None
    if "focal_gamma" in opts:
        return pkg.FocalLoss(opts["focal_gamma"])
    return torch.nn.CrossEntropyLoss(weight=torch.tensor(opts["weight"], device=DEV), label_smoothing=opts["label_smoothing"])


def _struct_bytes(s):
    return bytes(s)


# ---- the reference side's choices, one function each ------------------------------------------------------------------------------------
def _forward_weights(run, master):
    """{name: tensor} the train forward must have read: the quantiser's own tensors where it writes, the master's elsewhere."""
    if run.quant is None:
        return dict(master)
    return {k: run.quant._own[k] if k in run.quant.q else master[k] for k in master}


def _teacher_weights(before, teacher):
    """The teacher's weights the step must have used: those from before the step."""
    return before


def _grad_scale(trainer):
    return None if trainer.max_grad_norm is None else trainer._scale.clone()


def _ledger_rows(entries, labels, sel):
    return (entries, labels) if sel is None else (entries[sel], labels[sel])


def _average_source(master_after):
    """What the average follows: the master weights the Adam launch left."""
    return master_after


class _Run:
    """One configuration's trainer with everything around it, a twin for the module path, and the running expectations."""

    def __init__(self, name, T, max_grad_norm):
        c = self.c = sr.CONFIGS[name]
        self.name, self.T = name, T
        self.model, _ = tqat._golden_master(c["model"])
        m = self.model
        if c["select"] is not None and c["select"][1] is not None:
            # a head that leans towards the wake word by a mean margin of 1 on the first batch (p about 0.73: no loss so small that
            # torch's float32 focal loss, the reference of contract 5, loses its digits): the positives are then the EASY rows, the
            # loss alone would keep few of them, and keep_class=1 is what does
            with torch.no_grad():
                z = m.eval()(tt._batch(sr.BATCHES[0], T, seed=40)[0])
                m.train()
                lean = 0.5 * (1.0 - float((z[:, 1] - z[:, 0]).mean()))
                m.fc.bias.add_(torch.tensor([-lean, lean], device=DEV))
        self.quant = pkg.WeightQuant(m, bits=sr.BITS, clip=c["qat"]) if c["qat"] else None
        self.average = pkg.WeightAverage(m, decay=sr.DECAY) if c["average"] else None
        self.teacher = {"fixed": lambda: tt._model("full", seed=5).eval(), "mean": lambda: self.average.model, None: lambda: None}[c["teacher"]]()
        self.ledger = pkg.ClipLedger(sr.N_ENTRIES, DEV) if c["ledger"] else None
        kw = {}
        if c["teacher"]:
            kw.update(teacher=self.teacher, distill_alpha=c["alpha"], distill_temperature=c["temperature"])
        if c["qat"]:
            kw.update(quant=self.quant, qat=True, qat_calibrate=c["calibrate"])
        if c["select"]:
            kw.update(select=pkg.HardSelect(*c["select"]))
        self.trainer = pkg.WakewordTrainer(m, DEV, criterion=_criterion(c["opts"]), max_grad_norm=max_grad_norm, average=self.average,
                                           ledger=self.ledger, **kw)
        if self.ledger is not None:
            self.ledger.begin_epoch()
        self.named = dict(m.named_parameters())
        self.twin = tt.MODELS[c["model"]]().to(DEV).train()                       # the module path, dropout as the model's
        self.scorer = tt.MODELS[c["model"]]().to(DEV).train()                     # ... and without dropout: the scoring pass
        self.scorer.lstm.dropout, self.scorer.dropout.p = 0.0, 0.0
        self.lr = self.trainer.optimizer.param_groups[0]["lr"]
        self.wd = self.trainer.optimizer.param_groups[0]["weight_decay"]
        assert (self.lr, self.wd) == (pkg.TrainingConfig.LEARNING_RATE, sr.WEIGHT_DECAY)
        self.record = sr.new_ledger()
        self.stats = dict(correct=0, total=0, batches=0, bad_labels=0, nonfinite=0)
        self.loss_sum = 0.0
        self.dstats = dict(kd_rows=0, hard_rows=0, agree=0, teacher_correct=0, teacher_nonfinite=0, batches=0)
        self.sstats = None
        self.snaps, self.cut, self.scales, self.norms, self.mined, self.rescued = [], [], [], [], 0, 0

    def inputs(self, i, B):
        c = self.c
        x, y = tt._batch(B, self.T, seed=40 + i)
        labels = y[:, 0].clone()
        labels[sr.ignored_row(B)] = -100
        target = {"labels": labels, "probs": torch.from_numpy(sr.soft_targets(B, i)).to(DEV), None: None}[c["target"]]
        e = sr.entries_for(B, i)
        entries = None if c["ledger"] is None else torch.from_numpy(e).to(DEV) if c["ledger"] == "device" else e
        return x, target, entries, labels, e

    def opt_state(self):
        st = self.trainer.optimizer.state
        zeros = lambda p: torch.zeros_like(p)                                       # noqa: E731
        return ({k: st[p]["exp_avg"].detach().clone() if p in st and len(st[p]) else zeros(p) for k, p in self.named.items()},
                {k: st[p]["exp_avg_sq"].detach().clone() if p in st and len(st[p]) else zeros(p) for k, p in self.named.items()})

    def _load(self, module, tensors):
        with torch.no_grad():
            for k, p in module.named_parameters():
                p.copy_(tensors[k])
        module.zero_grad(set_to_none=True)

    # ---- one step and its nine contracts ----
    def step(self, i, B, calls, quiet=False):
        c, tr = self.c, self.trainer
        tag = f"{self.name} T={self.T} step {i + 1} (B={B})"
        x, target, entries, labels, e_host = self.inputs(i, B)
        master = {k: p.detach().clone() for k, p in self.named.items()}
        m0, v0 = self.opt_state()
        avg0 = {k: a.detach().clone() for k, a in self.average._avg.items()} if self.average is not None else None
        teacher0 = {k: v.detach().clone() for k, v in self.teacher.state_dict().items()} if self.teacher is not None else None
        d_before = ops.read_distill_stats(tr.distill_stats) if self.teacher is not None else None
        kwargs = {} if entries is None else {"entries": entries}
        if c["target"] != "labels":
            kwargs["labels"] = labels
        torch.cuda.synchronize()
        gc.collect()                                                                # nothing of an earlier test is freed inside the window
        n0 = len(calls)
        torch.manual_seed(SEED + i)
        if quiet and c["teacher"] != "mean":                                        # a mean teacher repacks through the host (section 3p)
            before = torch.cuda.memory_allocated()
            torch.cuda.set_sync_debug_mode("error")
            try:
                tr.step(x, target, **kwargs)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            assert torch.cuda.memory_allocated() == before, f"{tag}: the step allocated"
        else:
            tr.step(x, target, **kwargs)
        rng_after = torch.get_rng_state()
        step_calls = list(calls[n0:])
        torch.cuda.synchronize()
        k = sr.kept_of(c, B)
        mined = k < B
        calibrating = sr.calibrates(c, i)
        assert step_calls == sr.expected_launches(c, mined=mined, calibrating=calibrating), f"{tag}: launches {step_calls}"
        # the seed: ONE draw from torch's CPU generator, mined or not, rule or no rule
        torch.manual_seed(SEED + i)
        torch.randint(0, 2 ** 62, (1,), dtype=torch.int64)
        assert torch.equal(rng_after, torch.get_rng_state()), f"{tag}: the step did not draw exactly one seed"
        n_conv = tr._n_conv

        # ---- 1: the quantiser ----
        scale_dev = {}
        if self.quant is not None:
            wq = self.quant
            clips = {kk: _np(v) for kk, v in wq.clip.items()} if c["qat"] == "mse" else None
            read, scale = sr.quantised({kk: _np(v) for kk, v in master.items()}, clips, sr.BITS)
            for kk in wq.quantized:
                assert _bits_equal(_np(wq._own[kk]), read[kk]), f"{tag}: 1 quantiser, {kk}"
                assert _bits_equal(_np(wq.scale[kk]), scale[kk]), f"{tag}: 1 quantiser, scale of {kk}"
            want_tp = ops._train_params_struct([wq._own[kk] if kk in wq.q else self.named[kk] for kk in tr._keys], n_conv)
            assert _struct_bytes(tr._tp_q) == _struct_bytes(want_tp), f"{tag}: 1 the table of forward and backward"
            assert sorted(wq.quantized) == sorted(kk for kk, p in self.named.items() if p.dim() >= 2)
            if c["qat"] == "mse":
                scale_dev = {kk: _np(wq.scale[kk]) for kk in wq.quantized}
                assert wq.n_calibrations == 1 + sum(sr.calibrates(c, j) for j in range(i + 1)), f"{tag}: 1 calibrations"
        assert _struct_bytes(tr._tp) == _struct_bytes(ops._train_params_struct([self.named[kk] for kk in tr._keys], n_conv)), f"{tag}: the master's table"

        # ---- 2: scoring, selection, gather ----
        sel = None
        if mined:
            self._load(self.scorer, master)                                         # the RAW master weights
            s_out = self.scorer(x).detach()
            assert torch.equal(tr._slogits[:B], s_out), f"{tag}: 2 the scoring logits"
            scores, got_sel = _np(tr.last_scores), _np(tr.last_selected)
            keep_class = c["select"][1]
            want = sr.selection(_np(s_out), _np(target), c["opts"], k, keep_class, scores=scores)
            free = sr.selection(_np(s_out), _np(target), c["opts"], k, keep_class)
            ranked = want["rank"] > 0
            excess = float((np.abs(scores[ranked] - want["loss"][ranked]) - want["bound"][ranked]).max())
            print(f"{tag}: scores' largest (error - bound) {excess:.3e}; kept {got_sel.tolist()}")
            assert scores.shape == (B,) and excess <= 0.0 and np.isneginf(scores[~ranked]).all(), f"{tag}: 2 scores"
            assert got_sel.shape == (k,) and np.array_equal(got_sel, want["sel"]) and np.array_equal(got_sel, free["sel"]), f"{tag}: 2 last_selected"
            self.sstats = want["stats"] if self.sstats is None else {
                kk: want["stats"][kk] if kk == "threshold" else self.sstats[kk] + want["stats"][kk] for kk in want["stats"]}
            assert ops.read_select_stats(tr.select_stats) == self.sstats, f"{tag}: 2 select_stats"
            assert 0 < k < B and not np.array_equal(got_sel, np.arange(k)), f"{tag}: the selection is the first k rows"
            if keep_class is not None:
                self.rescued += len(set(got_sel.tolist()) - set(sr.selection(_np(s_out), _np(target), c["opts"], k, None, scores=scores)["sel"].tolist()))
            sel = torch.from_numpy(got_sel).to(DEV)
            g = tr._gathered
            assert torch.equal(g["x"][:k], x[sel]) and torch.equal(g["soft" if c["target"] == "probs" else "y"][:k], target[sel]), f"{tag}: 2 gather"
            if entries is not None:
                assert torch.equal(g["entries"][:k], torch.from_numpy(e_host).to(DEV)[sel]), f"{tag}: 2 gathered entries"
                assert c["target"] != "probs" or torch.equal(g["labels"][:k], labels[sel]), f"{tag}: 2 gathered labels"
            self.mined += 1
            x, target = x[sel].contiguous(), target[sel].contiguous()
        elif c["select"] is not None:
            assert self.sstats is None or ops.read_select_stats(tr.select_stats) == self.sstats, f"{tag}: an unmined step touched select_stats"

        # ---- 3: the train forward ----
        self._load(self.twin, _forward_weights(self, master))
        torch.manual_seed(SEED + i)
        out = self.twin(x)
        assert tr.last_logits.shape[0] >= k and torch.equal(tr.last_logits[:k], out.detach()), f"{tag}: 3 forward"
        z = _np(out)

        # ---- 4: the teacher ----
        zt = None
        if self.teacher is not None:
            packed = torch.from_numpy(ops.pack_state_dict(_teacher_weights(teacher0, self.teacher))).to(DEV)
            zt_want = ops.cnn_lstm_forward(x, packed, self.teacher._n_conv)
            assert tr.last_teacher_logits.shape == (k, 2) and torch.equal(tr.last_teacher_logits, zt_want), f"{tag}: 4 teacher"
            zt = _np(tr.last_teacher_logits)

        # ---- 5: loss, gradient, counters ----
        t_np = None if target is None else _np(target)
        want = sr.loss(z, zt, t_np, c["opts"], c["alpha"], c["temperature"])
        got_loss, d = float(tr.last_loss), _np(tr._dlogits[:k])
        if want["kind"] == "distill":
            e_loss, e_d = distill_ref.loss_excess(got_loss, want["loss"]), distill_ref.dlogits_excess(d, want["want"])
            print(f"{tag}: distillation (error - bound): loss {e_loss:.3e}, dlogits {e_d:.3e}")
            assert e_loss <= 0.0 and e_d <= 0.0, f"{tag}: 5 loss {got_loss!r} against {want['loss']!r}"
            d_now = ops.read_distill_stats(tr.distill_stats)
            for key in ("hard", "kd"):
                assert abs(d_now[key + "_sum"] - d_before[key + "_sum"] - want["want"][key]) <= distill_ref.loss_bound(want["want"][key]), f"{tag}: 5 {key}_sum"
            self.dstats = {kk: self.dstats[kk] + want["distill_stats"][kk] for kk in self.dstats}
            assert {kk: d_now[kk] for kk in self.dstats} == self.dstats, f"{tag}: 5 distill_stats {d_now}"
        else:
            case = {"opts": dict(c["opts"])}
            if want["kind"] == "soft":
                lt, dt = mixup_ref.torch_reference(case, z, t_np, DEV)
                caps = (mixup_ref.CAP_SOFT_LOSS, mixup_ref.CAP_SOFT_DLOGITS)
            else:
                lt, dt = loss_ref.torch_reference(case, z, t_np, DEV, pkg.FocalLoss)
                caps = (loss_ref.CAP_FOCAL_LOSS, loss_ref.CAP_FOCAL_DLOGITS) if want["kind"] == "focal" else (loss_ref.CAP_CE_LOSS, loss_ref.CAP_CE_DLOGITS)
            w = want["want"]
            tt._rule(f"{tag}: 5 loss", loss_ref.loss_error(got_loss, w["loss"]), loss_ref.loss_error(lt, w["loss"]), caps[0])
            tt._rule(f"{tag}: 5 dlogits", loss_ref.dlogits_error(d, w), loss_ref.dlogits_error(dt, w), caps[1])
        self.stats = {kk: self.stats[kk] + want["train_stats"][kk] for kk in self.stats}
        self.loss_sum += got_loss
        s = ops.read_loss_stats(tr.train_stats)
        assert {kk: s[kk] for kk in self.stats} == self.stats and s["loss_sum"] == self.loss_sum, f"{tag}: 5 train_stats {s}"
        assert self.stats["batches"] == i + 1 and self.stats["total"] == sum(sr.kept_of(c, b) for b in self.batches[:i + 1])

        # ---- 6: backward and mask ----
        out.backward(gradient=tr._dlogits[:k].clone())
        raw = {kk: _np(p.grad) for kk, p in self.twin.named_parameters()}
        cut_grads = sr.masked({kk: _np(v) for kk, v in master.items()}, scale_dev, raw, sr.BITS)
        for kk, p in self.named.items():
            assert _bits_equal(_np(p.grad), cut_grads[kk]), f"{tag}: 6 gradient of {kk}"
            assert p.grad is tr._grads[kk.replace("bias_hh", "bias_ih")], f"{tag}: {kk}.grad is not the trainer's buffer"
        cut = sum(int((cut_grads[kk].view(np.int32) != raw[kk].view(np.int32)).sum()) for kk in raw)
        self.cut.append(cut)

        # ---- 7: the norm ----
        grads_dev = {kk: _np(p.grad) for kk, p in self.named.items()}
        if tr.max_grad_norm is not None:
            n64, s64 = sr.clip(grads_dev, tr.max_grad_norm)
            got_n, got_s = float(tr._norm), float(tr._scale)
            n_raw = sr.clip(raw, tr.max_grad_norm)[0]
            print(f"{tag}: norm {got_n:.6f} (float64 {n64:.6f}, unmasked {n_raw:.6f}), scale {got_s:.6f}, {cut} gradient words cut")
            assert abs(got_n - n64) <= ref.norm_bound(n64), f"{tag}: 7 norm {got_n!r} against {n64!r}"
            if s64 == 1.0:
                assert got_s == 1.0, f"{tag}: 7 scale {got_s!r}: the clip is idle"
            else:
                assert got_s < 1.0 and abs(got_s - s64) <= ref.scale_bound(s64), f"{tag}: 7 scale {got_s!r} against {s64!r}"
            self.scales.append(got_s)
            self.norms.append((got_n, n64, n_raw))

        # ---- 8: Adam and the average ----
        names = list(self.named)
        t = i + 1
        ps, ms, vs = [master[kk].clone() for kk in names], [m0[kk].clone() for kk in names], [v0[kk].clone() for kk in names]
        gs = [self.named[kk].grad.clone() for kk in names]
        common = dict(lr=self.lr, betas=sr.BETAS, eps=sr.EPS, weight_decay=self.wd, step=t, grad_scale=_grad_scale(tr))
        if self.average is not None:
            avs = [avg0[kk].clone() for kk in names]
            ops.adam_average_step(ps, gs, ms, vs, avs, avg_weight=update_weight(i, "ema", sr.DECAY), **common)
        else:
            ops.adam_step(ps, gs, ms, vs, **common)
        torch.cuda.synchronize()
        m1, v1 = self.opt_state()
        for j, kk in enumerate(names):
            assert torch.equal(self.named[kk], ps[j]) and torch.equal(m1[kk], ms[j]) and torch.equal(v1[kk], vs[j]), f"{tag}: 8 Adam, {kk}"
            assert self.average is None or torch.equal(self.average._avg[kk], avs[j]), f"{tag}: 8 the average of {kk}"
            assert float(tr.optimizer.state[self.named[kk]]["step"]) == float(t), f"{tag}: 8 step count of {kk}"
        scale_now = 1.0 if tr.max_grad_norm is None else float(tr._scale)
        f64 = sr.update({"p": {kk: _np(v) for kk, v in master.items()}, "m": {kk: _np(v) for kk, v in m0.items()}, "v": {kk: _np(v) for kk, v in v0.items()}},
                        grads_dev, scale_now, t, self.lr, self.wd)
        tparams = {kk: torch.nn.Parameter(master[kk].clone()) for kk in names}
        topt = torch.optim.Adam(list(tparams.values()), lr=self.lr, weight_decay=self.wd, foreach=False)
        for kk, p in tparams.items():
            topt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": m0[kk].clone(), "exp_avg_sq": v0[kk].clone()}
            p.grad = self.named[kk].grad.clone() if tr.max_grad_norm is None else self.named[kk].grad * tr._scale
        topt.step()
        torchs = {"p": {kk: _np(p) for kk, p in tparams.items()}, "m": {kk: _np(topt.state[p]["exp_avg"]) for kk, p in tparams.items()},
                  "v": {kk: _np(topt.state[p]["exp_avg_sq"]) for kk, p in tparams.items()}}
        o, th, f = tt._all_errors(tt._state_of(self.model, tr.optimizer), torchs, f64, self.lr)
        tt._adam_rule(f"{tag}: 8", o, th, f, self.lr)
        self.snaps.append(torch.cat([p.detach().reshape(-1) for p in _average_source(self.model.parameters())]).clone())

        # ---- 9: the ledger ----
        if self.ledger is not None:
            rows_e, rows_y = _ledger_rows(e_host, _np(labels), None if sel is None else _np(sel))
            sr.ledger(self.record, rows_e, _np(tr.last_logits[:k]), rows_y, 0)
            assert self.ledger.read().tobytes() == self.record.tobytes(), f"{tag}: 9 ledger"
        return tag

    batches = sr.BATCHES + (sr.EXTRA_BATCH,)

    def check_average(self):
        """After the four steps: the averaged weights against the float64 recursion over the four snapshots the Adam launches left."""
        n = len(self.snaps)
        weights = sr.average_weights(n)
        assert weights == [update_weight(j, "ema", sr.DECAY) for j in range(n)] and self.average.n_averaged == n
        a64 = sr.average([_np(sn) for sn in self.snaps], weights)
        pmax = max(float(sn.abs().max()) for sn in self.snaps)
        ours = torch.cat([p.detach().reshape(-1) for p in self.average.model.parameters()])
        aref.rule(f"{self.name}: average over {n} steps", aref.error(_np(ours), a64, pmax), aref.error(_np(aref.lerp_reference(self.snaps, weights)), a64, pmax),
                  aref.CAP_SHORT)


def _dry_norm(name, T):
    """The float64 norm of step 1's gradients in a run of the same configuration without a clip."""
    dry = _Run(name, T, None)
    x, target, entries, labels, _ = dry.inputs(0, sr.BATCHES[0])
    kwargs = {} if entries is None else {"entries": entries}
    if dry.c["target"] != "labels":
        kwargs["labels"] = labels
    torch.manual_seed(SEED)
    dry.trainer.step(x, target, **kwargs)
    torch.cuda.synchronize()
    return sr.clip({k: _np(p.grad) for k, p in dry.named.items()}, 1.0)[0]


CASES = ([("qat_all", 8, m, "tight") for m in MATHS] + [("select_focal", 8, m, "tight") for m in MATHS]
         + [("qat_mean_teacher", 8, MATHS[0], "tight"), ("unlabelled", 8, MATHS[0], "tight"), ("select_soft", 8, MATHS[0], "tight"),
            ("qat_all", 32, MATHS[0], "tight"), ("qat_all", 8, MATHS[0], "loose")])


@pytest.mark.parametrize("name, T, math, norm", CASES, ids=[f"{n}-T{T}-{m}-{norm}" for n, T, m, norm in CASES])
def test_composed_step_meets_every_stage_contract(monkeypatch, name, T, math, norm):
    assert set(MATHS) <= set(ops.TRAIN_MATH)
    ops.set_train_math(math)
    try:
        n_dry = _dry_norm(name, T)
        run = _Run(name, T, n_dry * (0.5 if norm == "tight" else 1000.0))
        c, tr = run.c, run.trainer
        calls = tq._record(monkeypatch, sr.LAUNCHES)
        for i, B in enumerate(run.batches):
            if name == "qat_all" and i == 2:                                        # the rebinding path: QAT and the norm both on
                tr.optimizer.zero_grad(set_to_none=True)
                assert all(p.grad is None for p in run.named.values())
            run.step(i, B, calls, quiet=i in (2, 4))
            if i == 3 and run.average is not None:
                run.check_average()
        # ---- the conditions that make the contracts mean something ----
        assert len(run.scales) == len(run.batches)
        if norm == "tight":
            assert run.scales[0] < 1.0, f"{name}: step 1 does not exercise the clip (scale {run.scales[0]})"
            assert abs(run.norms[0][1] - n_dry) <= ref.norm_bound(n_dry)            # the dry run saw the same gradients
        else:
            assert all(s == 1.0 for s in run.scales), f"{name}: a loose max_grad_norm clipped ({run.scales})"
        if c["qat"] == "mse":
            assert run.quant.report().totals["saturated"] > 0 and all(n > 0 for n in run.cut), f"{name}: the mask changed nothing in a step ({run.cut})"
            if name == "qat_all":                                                   # the order is observable: the unmasked norm is another number
                assert all(abs(n_raw - got) > ref.norm_bound(n64) for got, n64, n_raw in run.norms), run.norms
        else:
            assert not any(run.cut)
        if c["select"] is not None:
            assert run.mined == sum(sr.kept_of(c, B) < B for B in run.batches) > 0
            assert c["select"][1] is None or run.rescued > 0, f"{name}: keep_class kept no row it would otherwise have dropped"
        if run.average is not None and c["qat"]:                                    # the average follows the master, not the fake-quant copy
            own = dict(run.quant.model.named_parameters())
            assert any(not torch.equal(run.named[k], own[k]) for k in run.quant.quantized)
    finally:
        monkeypatch.undo()
        ops.set_train_math("f16x3")
