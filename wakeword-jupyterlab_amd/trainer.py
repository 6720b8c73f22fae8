"""WakewordTrainer: the reference's training class (wakeword_training_script.py:219-348, notebook cell 9) with the whole batch on HIP.

Same constructor, attributes and methods -- `criterion`, `optimizer`, `scheduler`, the four history lists, `patience`, `best_val_acc`,
`epochs_no_improve`; `train_epoch`, `validate`, `train` -- and the same checkpoint dict.  What differs is what a batch costs: `step` calls
the C entry points directly, train forward -> the loss `criterion` names (loss, gradient, running metrics) -> backward -> optional gradient-norm clip
-> Adam, without autograd, without a torch kernel in between, without a device-to-host copy and, after the first call at a batch size,
without an allocation.  The epoch's loss and accuracy are kept on the device and read once, at the end of the epoch.

`validate` also keeps a clip-evaluation record on the device (ops.new_clip_metrics: confusion, operating points, margin histogram; one
more launch per batch, no wait); `trainer.val_report` reads it, lazily, as a metrics.ClipReport.  `monitor=` chooses what the scheduler,
the best checkpoint and early stopping follow: "val_acc" (the reference's behaviour, the default), "val_f1" (the wake-word class's F1
at argmax, times 100) or "val_auc" (the ROC AUC of the margins, times 100).

`ledger=` / `val_ledger=` (ledger.ClipLedger, also assignable as attributes) keep a per-clip record: `train_epoch` opens the ledger's next
epoch and scatters every step's train-mode logits by the loader's `last_entries`, `validate` does the same into `val_ledger` with the
eval-mode logits -- one more launch per batch, no wait.  With both None a step issues exactly the launches it
always issued.

A float32 target [B, 2] holds class probabilities (mixup through `processor.set_mixup`, soft relabelling): `step` / `train_epoch` then run
the soft cross-entropy (ww_ce_loss_soft_f32) in the loss's place, the launch count unchanged; `validate` keeps integer labels
(INTEGRATION.md section 3n).

`average=` (average.WeightAverage around the same model) keeps an EMA or SWA of the weights: an every="step"
average is written by the Adam launch itself (ww_adam_avg_step_f32 in ww_adam_step_f32's place -- `step` issues the same number of native
calls), an every="epoch" one is updated once after `train_epoch`.  `evaluate="average"` makes `validate`, `val_report`, the monitor, the
scheduler, early stopping and the best checkpoint follow `average.model`; the checkpoint gains "average_state_dict" when an average is set.

`quant=` (quant.WeightQuant around the model or around `average.model`) with `evaluate="quant"`: `validate`
re-quantises (one launch, no wait) and then it, `val_report`, the monitor, the scheduler, early stopping and the best checkpoint follow
`quant.model`, the fake-quant model -- the kept checkpoint is the one that survives quantisation.  The checkpoint gains "quant_state_dict"
when a quantiser is set.  Without one nothing here is reached.

`qat=True` (with `quant=WeightQuant(model, ...)` around the model that is trained) turns the step into
quantisation-aware training: ONE quantiser launch in front of the forward (`quant.update(weights_only=True)`), the train forward and
backward read a second parameter table -- `quant.model`'s fake-quant weights, and the master's own float32 biases unless the quantiser
quantises them too --, the gradients land in the master's `.grad` buffers as always, under clip="mse" ONE ww_quant_ste_f32 launch zeroes
the gradients of the weights the clipped scale saturates (under "max" nothing saturates and nothing is launched), and the gradient
norm and Adam move the float32 master weights.  `qat_calibrate` says when a clip="mse" quantiser searches its clip indices anew: "epoch"
(train_epoch, before its first batch), an integer n (every n steps) or None (never after construction).  Losses, a teacher, the average
(of the master weights), the ledgers and evaluate="quant" compose unchanged; `select=` raises NotImplementedError.  With qat=False a
step is launch for launch what it was.

`teacher=` (an eval-mode SimpleWakewordModel or WakewordModel on the same device, of either class; `average.model` gives the mean
teacher) turns the step into knowledge distillation: the teacher's eval forward on the same batch into a
persistent buffer, then ONE ww_distill_loss_f32 launch in the loss's place -- (1 - distill_alpha) * criterion + distill_alpha * T^2 * KD
at T = distill_temperature -- with integer labels, class probabilities or no target at all (`step(data, None)`: unlabelled audio).
`trainer.distill_stats` keeps the two terms apart on the device and `train_epoch` publishes them as `trainer.distill_report`.
`validate` and the checkpoint do not change.  Without a teacher nothing here is reached.

`select=` (mining.HardSelect, also assignable as an attribute) turns the step into online hard example mining:
with k = select.rows(B) < B the step first scores all B rows -- the train kernels' forward with both dropout probabilities 0, on the raw
parameters, so nothing is packed and nothing waits -- then ONE ww_hard_select_f32 launch ranks the rows by the criterion's own per-clip
loss, ONE ww_select_rows_f32 launch gathers the k hardest (data, target, entries, labels) into persistent buffers, and the step as it
always was runs on those k rows.  `train_stats`, the epoch's loss and accuracy and the ledger then speak of the KEPT rows only;
`trainer.select_stats` is the device record of what was kept, `train_epoch` publishes it as `trainer.select_report`, and
`trainer.last_selected` / `trainer.last_scores` are views of the newest step's choice.  Without `select`, or with k >= B, nothing here is
reached.  `select` together with a teacher raises NotImplementedError.

One deliberate difference: the reference calls `clip_grad_norm_` BEFORE `backward()`, where it clips the previous batch's gradients or
nothing, so the default here is no clipping; `max_grad_norm=1.0` gives the clip the call meant, after the
backward.
"""
from __future__ import annotations

import warnings

import torch
import torch.nn as nn

from . import _native as nat
from . import ops
from .config import TrainingConfig
from .model import SimpleWakewordModel, WakewordModel
from .optim import FusedAdam


MONITORS = ("val_acc", "val_f1", "val_auc")
MONITOR_NAMES = {"val_acc": "Acc", "val_f1": "F1", "val_auc": "AUC"}
EVALUATE = ("model", "average", "quant")


class WakewordTrainer:
    def __init__(self, model, device, config=TrainingConfig, *, checkpoint_path="best_wakeword_model.pth", max_grad_norm=None,
                 monitor="val_acc", thresholds=(0.8,), criterion=None, ledger=None, val_ledger=None, average=None, evaluate="model",
                 teacher=None, distill_alpha=0.5, distill_temperature=2.0, select=None, quant=None, qat=False, qat_calibrate="epoch"):
        if not isinstance(model, (SimpleWakewordModel, WakewordModel)):
            raise TypeError(f"WakewordTrainer drives the HIP training kernels of SimpleWakewordModel and WakewordModel; got {type(model).__name__}")
        from .loss import check_distillation
        self.distill_alpha, self.distill_temperature = check_distillation(distill_alpha, distill_temperature)
        self._check_teacher(teacher, model)
        self._check_select(select, teacher)
        if evaluate == "quant" and quant is None:
            raise ValueError("evaluate='quant' needs a quantiser: WakewordTrainer(..., quant=WeightQuant(model))")
        if quant is not None:
            from .quant import WeightQuant
            if not isinstance(quant, WeightQuant):
                raise TypeError(f"WakewordTrainer: quant must be a quant.WeightQuant or None, got {type(quant).__name__}")
        self._qat, self.qat_calibrate = self._check_qat(qat, qat_calibrate, quant, model, select)
        self._qat_steps = 0
        if any(p.device.type != "cuda" for p in model.parameters()):
            raise TypeError("WakewordTrainer: the model's parameters are on the CPU; this path has no CPU implementation (model.to('cuda'))")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"max_grad_norm {max_grad_norm}: expected a positive number or None")
        if monitor not in MONITORS:
            raise ValueError(f"monitor {monitor!r}: expected one of {MONITORS}")
        if evaluate not in EVALUATE:
            raise ValueError(f"evaluate {evaluate!r}: expected one of {EVALUATE}")
        if evaluate == "average" and average is None:
            raise ValueError("evaluate='average' needs an average: WakewordTrainer(..., average=WeightAverage(model))")
        if average is not None and any(average.average_of(p) is None for p in model.parameters()):
            raise ValueError("average: it was built around another model (WeightAverage(model) takes the model that is trained)")
        self.monitor = monitor
        self.evaluate = evaluate
        self.average = average                                         # average.WeightAverage or None
        self.quant = quant                                             # quant.WeightQuant or None
        self.model = model
        self.device = device
        self.config = config
        self.checkpoint_path = checkpoint_path
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.ledger = ledger                                           # ledger.ClipLedger or None: the per-clip record of train_epoch
        self.val_ledger = val_ledger                                   # ... and of validate

        # the reference's attribute; `step` and `validate` compute the same loss in ww_ce_loss_f32 / ww_ce_loss_ex_f32 (the property below)
        self.criterion = nn.CrossEntropyLoss().to(device) if criterion is None else criterion
        self.optimizer = FusedAdam(model.parameters(), lr=config.LEARNING_RATE, weight_decay=1e-5)
        self.optimizer.average = average                               # an every="step" average rides in the Adam launch
        self.scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(self.optimizer, mode="max", factor=0.5, patience=5)

        self.train_losses = []
        self.val_losses = []
        self.train_accuracies = []
        self.val_accuracies = []

        self.patience = 10
        self.best_val_acc = 0.0
        self.epochs_no_improve = 0
        self.monitor_history = []                                      # the monitored value of every epoch of `train`
        self.best_monitor = 0.0

        # ---- persistent device state of `step` ----
        self._n_conv = model._n_conv
        self._keys = ops._train_keys(self._n_conv)
        named = dict(model.named_parameters())
        self._params = [named[k] for k in self._keys]
        for p in self._params:
            ops._require_cuda_f32(p, "parameter")
            if not p.is_contiguous():
                raise RuntimeError("WakewordTrainer: a parameter is not contiguous")
        self._dev = self._params[0].device
        self._grads = {}
        self._bind_grads()
        self.train_stats = ops.new_loss_stats(self._dev)
        self.val_stats = ops.new_loss_stats(self._dev)
        self.val_metrics = ops.new_clip_metrics(self._dev, thresholds)
        self._val_report = None
        self._validated = False
        self.last_loss = torch.zeros((), device=self._dev, dtype=torch.float32)       # the newest batch's mean loss, on the device
        # ---- distillation: the teacher, its persistent forward buffers and the record of the two terms ----
        self.teacher = teacher
        self.distill_stats = self.distill_report = None
        self._tlogits = self._tws = None
        self._last_teacher_logits = None
        # ---- loss-ranked selection: the rule, the record of what it kept and the persistent buffers of the scoring pass and the gather ----
        self._select = select
        self.select_stats = self.select_report = None
        self._slogits = self._sel = self._scores = self._sel_ws = None
        self._gathered = {}
        self._last_selected = self._last_scores = None
        if teacher is not None:
            if any(p.device != self._dev for p in teacher.parameters()):
                raise RuntimeError(f"WakewordTrainer: the teacher must be on the student's device ({self._dev})")
            # one buffer behind both epoch records: train_epoch reads them in ONE device-to-host copy
            self._epoch_stats = torch.zeros(len(ops.LOSS_STATS_FIELDS) + len(ops.DISTILL_STATS_FIELDS), device=self._dev, dtype=torch.int64)
            self.train_stats = self._epoch_stats[:len(ops.LOSS_STATS_FIELDS)]
            self.distill_stats = self._epoch_stats[len(ops.LOSS_STATS_FIELDS):]
        else:
            # the same arrangement for the selection's record (a rule may be assigned later; without one the second half stays zero)
            self._epoch_stats = torch.zeros(len(ops.LOSS_STATS_FIELDS) + len(ops.SELECT_STATS_FIELDS), device=self._dev, dtype=torch.int64)
            self.train_stats = self._epoch_stats[:len(ops.LOSS_STATS_FIELDS)]
            self.select_stats = self._epoch_stats[len(ops.LOSS_STATS_FIELDS):]
        self._cap = 0                                                                  # clips the batch buffers hold
        self._logits = self._dlogits = None
        self._ws = None
        self._norm = self._scale = self._norm_ws = self._norm_tables = None
        if self.max_grad_norm is not None:
            self._norm = torch.zeros(1, device=self._dev, dtype=torch.float64)
            self._scale = torch.ones(1, device=self._dev, dtype=torch.float32)

    # ---- the loss: what `criterion` holds is what the fused step computes ----
    @property
    def criterion(self):
        """The loss of `step` and `validate`: an nn.CrossEntropyLoss (weight, label_smoothing, ignore_index, reduction "mean" or "sum") or
        a loss.FocalLoss (gamma, weight, ignore_index, reduction).  Assigning reads these attributes ONCE and copies the weight to the host
        (one device-to-host copy, at the assignment, not in the step): a later in-place change of the module or of its weight tensor is
        not seen until the criterion is assigned again.  Anything else raises TypeError, reduction="none" NotImplementedError -- at the
        assignment; nothing is silently ignored.  The default nn.CrossEntropyLoss() runs the plain ww_ce_loss_f32 launch, under which a
        label of -100 is a bad label; under any other criterion labels equal to its ignore_index are ignored."""
        return self._criterion

    @criterion.setter
    def criterion(self, module):
        from .loss import FocalLoss
        if isinstance(module, FocalLoss):
            opts = ops.loss_opts(module.weight, 0.0, module.ignore_index, module.reduction, module.gamma)
        elif type(module) is nn.CrossEntropyLoss:
            opts = ops.loss_opts(module.weight, module.label_smoothing, module.ignore_index, module.reduction, None)
        else:
            raise TypeError(f"WakewordTrainer.criterion: the fused step computes nn.CrossEntropyLoss or FocalLoss, not {type(module).__name__} "
                            "(a hand-written loop over ops.train_forward can use any loss)")
        self._criterion, self._loss_opts = module, opts
        self._no_target_opts = ops.loss_opts(reduction=module.reduction)      # an unlabelled distillation batch reads the reduction alone

    # ---- distillation ----
    @staticmethod
    def _check_teacher(teacher, model) -> None:
        """Refusals of a teacher that need no device: its class, the student itself, train mode, trainable parameters that are the
        student's (the optimiser would move the teacher with every step)."""
        if teacher is None:
            return
        if teacher is model:
            raise ValueError("WakewordTrainer: the teacher is the model that is trained (for a mean teacher pass WeightAverage(model).model)")
        if not isinstance(teacher, (SimpleWakewordModel, WakewordModel)):
            raise TypeError(f"WakewordTrainer: the teacher runs on the HIP inference kernels of SimpleWakewordModel and WakewordModel; "
                            f"got {type(teacher).__name__}")
        if teacher.training:
            raise RuntimeError("WakewordTrainer: the teacher is in train mode; call teacher.eval()")
        own = {p.untyped_storage().data_ptr() for p in model.parameters()}
        if any(p.requires_grad and p.untyped_storage().data_ptr() in own for p in teacher.parameters()):
            raise ValueError("WakewordTrainer: a trainable parameter of the teacher shares its storage with the student's")

    # ---- quantisation-aware training ----
    @staticmethod
    def _check_qat(qat, qat_calibrate, quant, model, select):
        """Refusals of the QAT options that need no device; returns (qat, qat_calibrate)."""
        if not isinstance(qat, bool):
            raise TypeError(f"qat {qat!r}: expected a bool")
        if not (qat_calibrate is None or qat_calibrate == "epoch"
                or (isinstance(qat_calibrate, int) and not isinstance(qat_calibrate, bool) and qat_calibrate >= 1)):
            raise ValueError(f"qat_calibrate {qat_calibrate!r}: expected 'epoch', a positive integer (steps) or None")
        if not qat:
            return False, qat_calibrate
        if quant is None:
            raise ValueError("qat=True needs a quantiser: WakewordTrainer(..., quant=WeightQuant(model), qat=True)")
        if quant.source is not model:
            raise ValueError("qat: the quantiser was built around another model (WeightQuant(model) takes the model that is trained)")
        if select is not None:
            raise NotImplementedError("WakewordTrainer: select= together with qat=True is not supported (mining under QAT is out of scope)")
        if quant.clip_mode == "mse" and quant.quantize_bias:
            raise NotImplementedError("WakewordTrainer: qat=True with clip='mse' and quantize_bias=True is not supported (the two biases of an "
                                      "LSTM layer share one gradient buffer, which cannot carry two masks)")
        return True, qat_calibrate

    @property
    def qat(self) -> bool:
        """Whether `step` trains through the quantiser (set at construction)."""
        return self._qat

    # ---- loss-ranked selection ----
    @staticmethod
    def _check_select(select, teacher) -> None:
        """Refusals of a selection rule that need no device: its class, and a teacher beside it."""
        if select is None:
            return
        from .mining import HardSelect
        if not isinstance(select, HardSelect):
            raise TypeError(f"WakewordTrainer: select must be a mining.HardSelect or None, got {type(select).__name__}")
        if teacher is not None:
            raise NotImplementedError("WakewordTrainer: select= together with teacher= is not supported (ranking rows by the distillation "
                                      "loss is not implemented); drop one of the two")

    @property
    def select(self):
        """The selection rule of `step` (mining.HardSelect) or None.  Assignable; a rule beside a teacher raises NotImplementedError."""
        return self._select

    @select.setter
    def select(self, rule):
        self._check_select(rule, self.teacher)
        if rule is not None and self._qat:
            raise NotImplementedError("WakewordTrainer: select= together with qat=True is not supported (mining under QAT is out of scope)")
        self._select = rule

    @property
    def last_selected(self):
        """The rows the newest mined step kept: int64 [k] in rising row index, a view of the persistent buffer (None before one)."""
        return self._last_selected

    @property
    def last_scores(self):
        """The newest mined step's scores, float64 [B]: the per-clip loss of every candidate row at dropout 0, -inf for a rank-0 row."""
        return self._last_scores

    def _gather_buffer(self, name, shape, dtype):
        """The first shape[0] rows of the persistent buffer `name`.  Like the logits' buffers it only grows: a smaller batch (an
        epoch's ragged last one) takes a view, and the batch after it finds the rows it had."""
        buf = self._gathered.get(name)
        if buf is None or tuple(buf.shape[1:]) != tuple(shape[1:]) or buf.shape[0] < shape[0]:
            self._gathered[name] = None                      # release before replacing
            buf = self._gathered[name] = torch.empty(shape, device=self._dev, dtype=dtype)
        return buf if buf.shape[0] == shape[0] else buf[:shape[0]]

    def _mine(self, x, y, soft, soft_opts, entries, ledger_y, B, k, math):
        """The scoring forward on all B rows (dropout 0: no seed is drawn, the raw parameters are read), the selection and the gather:
        returns the k kept rows of (x, y, entries, ledger_y) in persistent buffers.  Three native calls, no wait; no allocation after
        the first batch of a size.  The caller has made x's device current and sized self._ws for B rows."""
        if B > ops.SELECT_MAX_ROWS:
            raise ValueError(f"WakewordTrainer.step: select= takes batches of up to {ops.SELECT_MAX_ROWS} rows, got {B}")
        if self._slogits is None or self._slogits.shape[0] < B:
            self._slogits = self._sel = self._scores = self._sel_ws = None
            self._slogits = torch.empty((B, 2), device=self._dev, dtype=torch.float32)
            self._sel = torch.empty(B, device=self._dev, dtype=torch.int64)
            self._scores = torch.empty(B, device=self._dev, dtype=torch.float64)
            self._sel_ws = torch.empty(ops.hard_select_workspace_bytes(B), device=self._dev, dtype=torch.uint8)
        slogits = self._slogits if B == self._slogits.shape[0] else self._slogits[:B]
        ops.train_forward_into(x, self._tp, 0.0, 0.0, 0, math, self._ws, slogits)
        sel = self._sel[:k]
        ops.hard_select_into(slogits, y, k, sel, self._scores, self.select_stats, self._sel_ws,
                             opts=soft_opts if soft else self._loss_opts, keep_class=self._select.keep_class)
        self._last_selected, self._last_scores = sel, self._scores[:B]
        want_ledger = entries is not None and self.ledger is not None
        if want_ledger and not isinstance(entries, torch.Tensor):
            entries = self.ledger._upload(entries, B)        # host integers: the ledger's own pinned staging, no wait
        gx = self._gather_buffer("x", (k,) + tuple(x.shape[1:]), torch.float32)
        gy = self._gather_buffer("soft" if soft else "y", (k, 2) if soft else (k,), y.dtype)
        ge = self._gather_buffer("entries", (k,), torch.int64) if want_ledger else None
        gl = self._gather_buffer("labels", (k,), torch.int64) if want_ledger and soft else None
        ops.select_rows_into(x, sel, gx, y, gy, entries if want_ledger else None, ge, ledger_y if gl is not None else None, gl)
        return gx, gy, ge if want_ledger else entries, gl if gl is not None else gy

    @staticmethod
    def _select_report(s) -> dict:
        """An epoch's ww_select_stats as what one reads off it: the fraction of the candidate rows that were trained on, the share of
        positives (counting rows of class 1) among the candidates and among the kept, the rank-0 rows (ignored or bad targets, non-finite
        logits) seen and kept, the smallest kept score of the newest mined step, and the counts behind them."""
        nan = float("nan")
        return {"kept_fraction": s["kept"] / s["candidates"] if s["candidates"] else nan,
                "candidate_positive_fraction": s["candidate_positive"] / s["candidates"] if s["candidates"] else nan,
                "kept_positive_fraction": s["kept_positive"] / s["kept"] if s["kept"] else nan,
                "unranked": s["unranked"], "kept_unranked": s["kept_unranked"], "threshold": s["threshold"],
                "candidates": s["candidates"], "kept": s["kept"], "candidate_positive": s["candidate_positive"],
                "kept_positive": s["kept_positive"], "batches": s["batches"]}

    def _teacher_forward(self, x, B):
        """The teacher's eval-mode logits of `x` in the persistent buffer: ww_model_forward_f32 on a persistent workspace, on the current
        stream; the caller has made x's device current.  The packed weights are the teacher's own cache (model.packed_weights): built
        once for a fixed teacher, rebuilt after every update of a mean teacher."""
        t = self.teacher
        if t.training:
            raise RuntimeError("WakewordTrainer.step: the teacher is in train mode; call teacher.eval()")
        need = ops.forward_workspace_bytes(B, t._n_conv)
        if self._tws is None or self._tws.numel() < need:
            self._tws = None
            self._tws = torch.empty(need, device=self._dev, dtype=torch.uint8)
        if self._tlogits is None or self._tlogits.shape[0] < self._cap:
            self._tlogits = torch.empty((self._cap, 2), device=self._dev, dtype=torch.float32)
        out = self._tlogits if B == self._tlogits.shape[0] else self._tlogits[:B]
        ops.model_forward_into(x, t.packed_weights(), t._n_conv, self._tws, out)
        return out

    @property
    def last_teacher_logits(self):
        """The newest step's teacher logits [B, 2]: a view of the persistent buffer, or the `teacher_logits=` the step was given."""
        return self._last_teacher_logits

    # ---- gradients: one persistent buffer per parameter, bound once ----
    def _bind_grads(self) -> None:
        """p.grad of every parameter is a buffer the backward kernel writes.  bias_hh_l*.grad IS bias_ih_l*.grad (the two gradients are
        equal); weight_hh_l*.grad is zeroed here and never written (h0 = 0 makes it exactly zero) -- Adam's weight decay still reaches
        weight_hh through it, as in the reference."""
        for k, p in zip(self._keys, self._params):
            if k.startswith("lstm.bias_hh"):
                continue
            if k not in self._grads:
                self._grads[k] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            p.grad = self._grads[k]
        for k, p in zip(self._keys, self._params):
            if k.startswith("lstm.bias_hh"):
                p.grad = self._grads[k.replace("bias_hh", "bias_ih")]
        self._tg = ops.train_grads_struct(self._grads, self._n_conv)
        self._tp = ops._train_params_struct(self._params, self._n_conv)
        self._tp_key = tuple(p.data_ptr() for p in self._params)
        if self._qat:
            self._bind_qat()

    def _bind_qat(self) -> None:
        """The second parameter table of a QAT step -- the fake-quant model's tensors where the quantiser writes them, the master's own
        elsewhere (the float32 biases) -- and, under clip="mse", the table of the straight-through launch over the master's gradients."""
        wq = self.quant
        self._tp_q = ops._train_params_struct([wq._own[k] if k in wq.q else p for k, p in zip(self._keys, self._params)], self._n_conv)
        grads = {k: p.grad for k, p in zip(self._keys, self._params)}
        self._ste_tables = wq.ste_tables(grads) if wq.clip_mode == "mse" else []
        self._qat_stats = wq._stats                          # the buffer behind the scales the tables point at: held, and watched by `step`

    def _grads_bound(self) -> bool:
        for k, p in zip(self._keys, self._params):
            if p.grad is not self._grads[k.replace("bias_hh", "bias_ih")]:
                return False
        return self._tp_key == tuple(p.data_ptr() for p in self._params)

    def _norm_step(self) -> None:
        """Global L2 norm over every parameter's gradient (a bias gradient counts for both its parameters, as clip_grad_norm_ counts
        it) -> self._norm and self._scale, on the device.  The two models have 14 and 16 parameters: one table."""
        if self._norm_tables is None:
            self._norm_tables = ops.adam_table(None, [p.grad for p in self._params], None, None)
            self._norm_ws = ops.grad_norm_workspace(self._norm_tables, self._dev)
        ops.grad_norm_launch(self._norm_tables, self._dev, self.max_grad_norm, self._norm, self._scale, self._norm_ws)

    def _target(self, target, B, soft=False):
        if not isinstance(target, torch.Tensor):
            raise TypeError(f"target: expected a torch.Tensor, got {type(target).__name__}")
        if target.device != self._dev:
            target = target.to(self._dev)
        if target.dtype == torch.float32 and soft:
            # class probabilities [B, 2] (mixup, soft relabelling): the soft cross-entropy of the fused step, or the hard term beside a teacher
            if target.dim() != 2 or tuple(target.shape) != (B, 2):
                raise ValueError(f"target: expected float32 class probabilities [{B}, 2], got {tuple(target.shape)}")
            return target if target.is_contiguous() else target.contiguous()
        if target.dtype != torch.int64:
            if target.dtype.is_floating_point or target.dtype == torch.bool:
                if target.dtype.is_floating_point and not soft:
                    raise TypeError(f"target: validate needs integer class labels (the clip metrics count hard labels), got {target.dtype}; "
                                    "class-probability targets are for step / train_epoch")
                raise TypeError(f"target: expected integer class labels or float32 class probabilities [B, 2], got {target.dtype}")
            target = target.to(torch.int64)
        if target.dim() == 2 and target.shape[1] == 1:
            target = target[:, 0]
        if target.dim() != 1 or target.shape[0] != B:
            raise ValueError(f"target: expected [{B}] or [{B}, 1], got {tuple(target.shape)}")
        return target if target.stride(0) == 1 or B == 1 else target.contiguous()

    @staticmethod
    def _entries_of(loader):
        """The bank entries (or file indices) of the batch `loader` has just yielded."""
        entries = getattr(loader, "last_entries", None)
        if entries is None:
            raise TypeError(f"a ledger needs a loader that names its rows: {type(loader).__name__} has no `last_entries` "
                            "(bank.loader() and dataset.loader() set it; a hand-written loop passes step(..., entries=))")
        return entries

    def _soft_opts(self):
        """The criterion's options as ww_ce_loss_soft_f32 takes them (None: the defaults); refusals before any launch."""
        from .loss import FocalLoss
        if isinstance(self._criterion, FocalLoss):
            raise NotImplementedError("WakewordTrainer.step: class-probability targets with a FocalLoss criterion are not supported "
                                      "(the focal loss takes integer labels); use nn.CrossEntropyLoss")
        if int(self._criterion.ignore_index) != -100:
            raise ValueError(f"WakewordTrainer.step: ignore_index {self._criterion.ignore_index} with class-probability targets "
                             "(torch refuses it too); leave it at -100")
        return self._loss_opts

    def step(self, data, target, entries=None, labels=None, teacher_logits=None) -> torch.Tensor:
        """One training batch: data [B, 1, 80, T <= 32] float32 and target [B] or [B, 1] int64, both on the GPU (tensors elsewhere, or of
        another integer type, are copied first).  A float32 target [B, 2] holds class probabilities (mixup: what a loader yields under
        `processor.set_mixup`; soft relabelling): the step then launches ww_ce_loss_soft_f32 in place of the integer-label loss -- the same
        number of launches, no wait, no allocation; `labels` [B] int64 on the device (train_epoch passes the loader's `last_labels`) are
        then what the ledger records.  Returns the batch's mean loss as a 0-d tensor ON THE DEVICE (self.last_loss, overwritten
        by the next step); the running metrics are in self.train_stats.  The model must be in train mode.  `entries` [B] (a host integer
        array or an int64 device tensor; train_epoch passes the loader's `last_entries`): with `self.ledger` set, the step's train-mode
        logits and labels are added to it under these entries, one more launch after the optimiser's.

        With a teacher (`teacher_logits`: float32 [B, 2] on the device, precomputed -- an ensemble, a teacher at another precision --
        then take the teacher forward's place) the loss launch is ww_distill_loss_f32: (1 - distill_alpha) * criterion +
        distill_alpha * T^2 * KD on integer labels or class probabilities, and on `target=None` (unlabelled audio) T^2 * KD alone.
        Integer labels then follow the rule of a criterion WITH options even under the default one: a label of -100 is ignored.

        With `self.select` set and k = select.rows(B) < B the batch is first scored without dropout, and everything above -- loss,
        gradient, train_stats, last_logits, the ledger's rows -- is about the k rows `self.last_selected` names (section 3r).

        With qat=True the quantiser runs first (one launch), forward and backward read the fake-quant weights, and under clip="mse" one
        more launch after the backward cuts the gradients of saturated weights (section 3t); the seed is drawn as always."""
        if not self.model.training:
            raise RuntimeError("WakewordTrainer.step: the model is in eval mode (train_epoch calls model.train())")
        if isinstance(data, torch.Tensor) and data.device != self._dev:
            data = data.to(self._dev)
        if isinstance(data, torch.Tensor) and data.dim() == 4 and data.shape[3] > 32:
            raise NotImplementedError(f"training at T = {data.shape[3]} frames is not supported yet: the training kernels take 1..32 "
                                      "(clips of up to 1 s); clips of up to 2 s run in eval mode only")
        x = ops._check_x(data)
        B = x.shape[0]
        if B == 0:
            raise ValueError("empty training batch")
        distill = self.teacher is not None
        k = B if self._select is None else self._select.rows(B)
        if k < B and distill:
            raise NotImplementedError("WakewordTrainer.step: select= together with a teacher is not supported")
        if not distill and (target is None or teacher_logits is not None):
            raise TypeError("WakewordTrainer.step: target=None (an unlabelled batch) and teacher_logits= need a teacher: "
                            "WakewordTrainer(..., teacher=)")
        y = None if target is None else self._target(target, B, soft=True)
        soft = y is not None and y.dtype == torch.float32
        soft_opts = self._soft_opts() if soft else None
        if teacher_logits is not None:
            if (not isinstance(teacher_logits, torch.Tensor) or teacher_logits.dtype != torch.float32 or teacher_logits.device != self._dev
                    or tuple(teacher_logits.shape) != (B, 2) or not teacher_logits.is_contiguous()):
                raise ValueError(f"teacher_logits: expected a contiguous float32 [{B}, 2] tensor on {self._dev}")
        ledger_y = y
        if y is None and entries is not None and self.ledger is not None:
            if labels is None:
                raise TypeError("a ledger on an unlabelled batch needs the rows' integer labels: step(..., labels=)")
            ledger_y = self._target(labels, B)
        if soft and entries is not None and self.ledger is not None:
            if labels is None:
                raise TypeError("a ledger with class-probability targets needs the rows' integer labels: step(..., labels=) "
                                "(bank.loader() and dataset.loader() set `last_labels`)")
            ledger_y = self._target(labels, B)
        if not self._grads_bound():                          # optimizer.zero_grad() or a .to(): bind the buffers again
            self._bind_grads()
            self._norm_tables = None
        tp = self._tp
        if self._qat:
            wq = self.quant
            if wq._stats is not self._qat_stats:             # load_state_dict changed the quantiser's grouping or clip mode: new buffers
                self._bind_qat()
            if wq.clip_mode == "mse" and isinstance(self.qat_calibrate, int) and self._qat_steps > 0 and self._qat_steps % self.qat_calibrate == 0:
                wq.calibrate()                               # the search, then the full update
            else:
                wq.update(weights_only=True)                 # one launch, no wait: the forward below reads the master's own biases
            self._qat_steps += 1
            tp = self._tp_q
        # the dropout seed exactly as _CnnLstm.forward draws it: one randint from torch's CPU generator
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        math = nat.lib.ww_get_train_math()                   # resolved once: query, forward and backward of this step get this value
        need = ops.train_workspace_bytes(B, self._n_conv, math)
        with torch.cuda.device(self._dev):
            if self._ws is None or self._ws.numel() < need:
                self._ws = None                              # release before growing
                self._ws = torch.empty(need, device=self._dev, dtype=torch.uint8)
            if B > self._cap:
                self._logits = torch.empty((B, 2), device=self._dev, dtype=torch.float32)
                self._dlogits = torch.empty((B, 2), device=self._dev, dtype=torch.float32)
                self._cap = B
            if k < B:
                x, y, entries, ledger_y = self._mine(x, y, soft, soft_opts, entries, ledger_y, B, k, math)
                B = k
            logits, m = self._logits if B == self._cap else self._logits[:B], self.model         # the buffers may hold more rows
            ops.train_forward_into(x, tp, m.lstm.dropout, m.dropout.p, seed, math, self._ws, logits)
            if distill:
                zt = self._teacher_forward(x, B) if teacher_logits is None else teacher_logits
                self._last_teacher_logits = zt
                ops.distill_loss_into(logits, zt, y, self._dlogits, self.last_loss, self.train_stats, self.distill_stats,
                                      alpha=self.distill_alpha, temperature=self.distill_temperature,
                                      opts=self._no_target_opts if y is None else soft_opts if soft else self._loss_opts)
            elif soft:
                ops.soft_ce_loss_into(logits, y, self._dlogits, self.last_loss, self.train_stats, opts=soft_opts)
            else:
                ops.ce_loss_into(logits, y, self._dlogits, self.last_loss, self.train_stats, opts=self._loss_opts)
            ops.train_backward_into(x, tp, self._dlogits, math, self._ws, self._tg)
            if self._qat:
                for tab in self._ste_tables:                 # clip="mse" alone: under "max" nothing saturates
                    ops.quant_ste_launch(tab, self._dev, self.quant.bits)
            if self.max_grad_norm is not None:
                self._norm_step()
        self.optimizer.step(grad_scale=self._scale if self.max_grad_norm is not None else None)
        if entries is not None and self.ledger is not None:
            self.ledger.update(entries, logits, ledger_y)
        return self.last_loss

    @property
    def last_logits(self) -> torch.Tensor:
        """The newest step's train-mode logits [B, 2] (a view of the persistent buffer, overwritten by the next step)."""
        return self._logits

    def _finish_epoch(self, stats, what):
        s = ops.read_loss_stats(stats)                       # the epoch's one device-to-host copy
        if s["bad_labels"] > 0:
            raise ValueError(f"{what}: {s['bad_labels']} of {s['total']} labels lie outside {{0, 1}} (they were left out of loss and gradient)")
        if s["nonfinite"] > 0:
            warnings.warn(f"{what}: {s['nonfinite']} of {s['total']} clips had a non-finite logit", RuntimeWarning, stacklevel=3)
        if s["batches"] == 0:
            raise ValueError(f"{what}: the loader gave no batch")
        return s["loss_sum"] / s["batches"], 100.0 * s["correct"] / s["total"]

    @staticmethod
    def _distill_report(d) -> dict:
        """An epoch's ww_distill_stats as what one reads off it: the mean of the batches' hard and KD terms (neither weighted by
        alpha; T^2 inside the KD term), the student-teacher agreement over the KD rows and the teacher's accuracy over the labelled
        rows in percent (NaN without such rows), the rows with a non-finite teacher logit, and the counts behind them."""
        nan = float("nan")
        return {"hard_loss": d["hard_sum"] / d["batches"] if d["batches"] else nan,
                "kd_loss": d["kd_sum"] / d["batches"] if d["batches"] else nan,
                "agreement": 100.0 * d["agree"] / d["kd_rows"] if d["kd_rows"] else nan,
                "teacher_accuracy": 100.0 * d["teacher_correct"] / d["hard_rows"] if d["hard_rows"] else nan,
                "teacher_nonfinite": d["teacher_nonfinite"], "kd_rows": d["kd_rows"], "hard_rows": d["hard_rows"], "batches": d["batches"]}

    def train_epoch(self, train_loader):
        self.model.train()
        self.train_stats.zero_()
        if self.teacher is not None:
            self.distill_stats.zero_()
        mined = self._select is not None and self.select_stats is not None
        if mined:
            self.select_stats.zero_()
        if self.ledger is not None:
            self.ledger.begin_epoch()
        if self._qat and self.qat_calibrate == "epoch" and self.quant.clip_mode == "mse":
            self.quant.calibrate()
        for data, target in train_loader:
            if self.ledger is None:
                self.step(data, target)
            else:
                self.step(data, target, self._entries_of(train_loader), getattr(train_loader, "last_labels", None))
        if mined:
            host = self._epoch_stats.cpu()                   # both records in the epoch's one device-to-host copy
            result = self._finish_epoch(host[:len(ops.LOSS_STATS_FIELDS)], "train_epoch")
            self.select_report = self._select_report(ops.read_select_stats(host[len(ops.LOSS_STATS_FIELDS):]))
        elif self.teacher is None:
            result = self._finish_epoch(self.train_stats, "train_epoch")
        else:
            host = self._epoch_stats.cpu()                   # both records in the epoch's one device-to-host copy
            result = self._finish_epoch(host[:len(ops.LOSS_STATS_FIELDS)], "train_epoch")
            self.distill_report = self._distill_report(ops.read_distill_stats(host[len(ops.LOSS_STATS_FIELDS):]))
        if self.average is not None and self.average.every == "epoch":
            self.average.update()
        return result

    def validate(self, val_loader):
        self.model.eval()
        if self.evaluate == "quant":
            self.quant.update()                              # from its source's current weights: one launch, no wait
            model = self.quant.model.eval()
        else:
            model = self.average.model.eval() if self.evaluate == "average" else self.model
        self.val_stats.zero_()
        ops.reset_clip_metrics(self.val_metrics)
        self._val_report = None
        self._validated = True
        if self.val_ledger is not None:
            self.val_ledger.begin_epoch()
        with torch.no_grad():
            for data, target in val_loader:
                if data.device != self._dev:
                    data = data.to(self._dev)
                output = model(data)
                y = self._target(target, output.shape[0])
                ops.ce_loss_into(output, y, None, None, self.val_stats, opts=self._loss_opts)
                ops.clip_metrics_update_into(output, y, self.val_metrics)
                if self.val_ledger is not None:
                    self.val_ledger.update(self._entries_of(val_loader), output, y)
        return self._finish_epoch(self.val_stats, "validate")

    @property
    def val_report(self):
        """The newest `validate` as a metrics.ClipReport, read from the device on first access (one copy) and kept until the next one."""
        if not self._validated:
            raise RuntimeError("WakewordTrainer.val_report: validate() has not run yet")
        if self._val_report is None:
            self._val_report = ops.read_clip_metrics(self.val_metrics)
        return self._val_report

    def _monitored(self, val_acc):
        if self.monitor == "val_acc":
            return val_acc                                   # no copy: the report stays on the device unless somebody reads it
        if self.monitor == "val_f1":
            return 100.0 * self.val_report.f1
        auc = self.val_report.auc
        if auc != auc:
            raise ValueError("monitor='val_auc': the validation set needs clips of both classes with finite logits")
        return 100.0 * auc

    def train(self, train_loader, val_loader, epochs):
        print(f"Starting training for {epochs} epochs...")
        print(f"Using device: {self.device}")
        print(f"Learning rate: {self.config.LEARNING_RATE}")
        print(f"Batch size: {self.config.BATCH_SIZE}")

        self.best_val_acc = 0.0
        self.best_monitor = 0.0
        self.epochs_no_improve = 0
        epoch = -1
        for epoch in range(epochs):
            print(f"\nEpoch {epoch + 1}/{epochs}")
            print(f"GPU Memory: {torch.cuda.memory_allocated() / 1e6:.1f}MB allocated, {torch.cuda.memory_reserved() / 1e6:.1f}MB reserved")

            train_loss, train_acc = self.train_epoch(train_loader)
            val_loss, val_acc = self.validate(val_loader)
            self.train_losses.append(train_loss)
            self.val_losses.append(val_loss)
            self.train_accuracies.append(train_acc)
            self.val_accuracies.append(val_acc)
            print(f"Train Loss: {train_loss:.4f}, Train Acc: {train_acc:.2f}%")
            print(f"Val Loss: {val_loss:.4f}, Val Acc: {val_acc:.2f}%")

            monitored = self._monitored(val_acc)
            self.monitor_history.append(monitored)
            if self.monitor != "val_acc":
                print(f"Val {MONITOR_NAMES[self.monitor]}: {monitored:.2f}%")

            self.scheduler.step(monitored)

            if monitored > self.best_monitor:
                self.best_monitor = monitored
                self.best_val_acc = val_acc                  # the accuracy of the best epoch by the monitor
                self.epochs_no_improve = 0
                ckpt = {"epoch": epoch, "model_state_dict": self.model.state_dict(), "optimizer_state_dict": self.optimizer.state_dict(),
                        "val_acc": val_acc, "train_acc": train_acc, "train_loss": train_loss, "val_loss": val_loss}
                if self.average is not None:
                    ckpt["average_state_dict"] = self.average.state_dict()
                if self.quant is not None:
                    if self.evaluate != "quant":
                        self.quant.update()                  # validate did not: the saved integers belong to the saved weights
                    ckpt["quant_state_dict"] = self.quant.state_dict()
                torch.save(ckpt, self.checkpoint_path)
                print(f"New best model saved! Validation accuracy: {val_acc:.2f}%")
            else:
                self.epochs_no_improve += 1

            if self.epochs_no_improve >= self.patience:
                print(f"\nEarly stopping triggered! No improvement for {self.patience} epochs.")
                print(f"Best validation accuracy: {self.best_val_acc:.2f}%")
                break

        print("\nTraining completed!")
        print(f"Best validation accuracy: {self.best_val_acc:.2f}%")
        print(f"Total epochs trained: {epoch + 1}")
        return self.best_val_acc
