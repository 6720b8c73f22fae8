"""WeightAverage: an averaged copy of a model's weights, kept on the GPU by the Adam launch itself.

An exponential moving average (EMA) or an equal-weight average over the late part of training (stochastic weight averaging, SWA) is what
keyword-spotting recipes evaluate, checkpoint and deploy: it costs nothing at inference and its validation curve is steadier than the
raw weights' -- which is what ReduceLROnPlateau, the best checkpoint and early stopping follow.

The arithmetic has one definition (include/wakeword_amd.h, ww_adam_avg_step_f32): with w = update_weight(n, ...) computed here in double,
a <- torch.lerp(a, p, w), each branch one fma; w = 1 (the first update) copies p without reading a, w = 0 touches nothing.  Where it runs:

  optim.FusedAdam.average     every="step" averages ride in the Adam launch (ww_adam_avg_step_f32): no launch of their own
  WakewordTrainer(average=)   the same through the trainer; every="epoch" averages are updated once after train_epoch
  WeightAverage.update()      on its own, one launch per 16 tensors (ww_weight_average_f32): any optimiser, any schedule

`update_weight` and the two state-dict conversions are pure host code: they work without a GPU.  Out of scope: optimiser state,
BatchNorm statistics (the models have none), averaging across GPUs.
"""
from __future__ import annotations

import copy
from collections import OrderedDict

import torch

MODES = ("ema", "swa")
EVERY = ("step", "epoch")


def update_weight(n: int, mode: str = "ema", decay: float = 0.999, warmup: bool = False) -> float:
    """The weight w of the update after `n` updates have been applied, in double: a <- a + w (p - a).
      n == 0        1.0, for both modes: the average becomes a copy of the parameters
      mode="ema"    1 - d with d = decay, or d = min(decay, (1 + n) / (10 + n)) under warmup -- without warmup this is
                    torch.optim.swa_utils.AveragedModel(..., multi_avg_fn=get_ema_multi_avg_fn(decay))
      mode="swa"    1 / (n + 1): the running equal-weight mean, torch's get_swa_avg_fn"""
    if mode not in MODES:
        raise ValueError(f"mode {mode!r}: expected one of {MODES}")
    if isinstance(n, bool) or int(n) != n or n < 0:
        raise ValueError(f"n {n!r}: expected the number of updates already applied, an integer >= 0")
    if n == 0:
        return 1.0
    if mode == "swa":
        return 1.0 / (float(n) + 1.0)
    d = float(decay)
    if not 0.0 <= d <= 1.0:
        raise ValueError(f"decay {decay!r}: expected a value in [0, 1]")
    if warmup:
        d = min(d, (1.0 + n) / (10.0 + n))
    return 1.0 - d


class WeightAverage:
    """The averaged weights of `model`.

    .model        a module of the model's own class whose parameters ARE the averaged tensors: in eval mode, without gradients, on the
                  model's device; forward, forward_pcm, StreamingDetector, scan_files and save_deployment_package take it as they take
                  any model.  Until the first update it holds a copy of the model's weights.
    .n_averaged   updates applied so far, a host integer
    .update()     one update on its own (see the module text); FusedAdam and WakewordTrainer call the fused form instead

    every="step" | "epoch" says what one update stands for -- and so what `start` counts: the first `start` updates (steps or epochs)
    are skipped, which is how SWA over the late epochs is written: WeightAverage(model, mode="swa", every="epoch", start=20).
    After every update the averaged tensors' version counters move as for an in-place op, so `.model.packed_weights()` rebuilds."""

    def __init__(self, model, mode="ema", decay=0.999, warmup=False, every="step", start=0):
        if not isinstance(model, torch.nn.Module):
            raise TypeError(f"WeightAverage: expected an nn.Module, got {type(model).__name__}")
        self._configure(mode, decay, warmup, every, start)
        self.n_averaged = 0
        self.n_calls = 0                                     # updates asked for, the skipped ones before `start` included
        self.source = model
        self.model = copy.deepcopy(model)
        self.model.eval()
        if hasattr(self.model, "_packed"):
            self.model._packed = self.model._packed_key = None          # the copy packs its own weights on first use
        for p in self.model.parameters():
            p.requires_grad_(False)
            p.grad = None
        self._avg = dict(self.model.named_parameters())
        self._names = list(self._avg)
        self._bound = [p for _, p in model.named_parameters()]
        self._by_param = {id(p): self._avg[k] for k, p in zip(self._names, self._bound)}     # id(source parameter) -> its averaged tensor
        self._tables = {}                                    # (pointers of a launch's tensors) -> its ctypes table and pointer array

    def _configure(self, mode, decay, warmup, every, start):
        if mode not in MODES:
            raise ValueError(f"mode {mode!r}: expected one of {MODES}")
        if every not in EVERY:
            raise ValueError(f"every {every!r}: expected one of {EVERY}")
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"decay {decay!r}: expected a value in [0, 1]")
        if isinstance(start, bool) or int(start) != start or start < 0:
            raise ValueError(f"start {start!r}: expected an integer >= 0")
        self.mode, self.decay, self.warmup, self.every, self.start = mode, float(decay), bool(warmup), every, int(start)

    # ---- what FusedAdam asks ----
    def average_of(self, param):
        """The averaged tensor of one of the source model's parameters, or None."""
        return self._by_param.get(id(param))

    def pairs(self):
        """[(parameter, its averaged tensor)] of the source model, in named_parameters order."""
        return [(p, self._avg[k]) for k, p in zip(self._names, self._bound)]

    def next_weight(self):
        """The weight of the update that is due, or None while the first `start` updates are being skipped."""
        if self.n_calls < self.start:
            return None
        return update_weight(self.n_averaged, self.mode, self.decay, self.warmup)

    def advance(self, applied: bool) -> None:
        """Count one update: `applied` False for a skipped one."""
        self.n_calls += 1
        if applied:
            self.n_averaged += 1

    @staticmethod
    def touched(tensors) -> None:
        """A kernel wrote these averaged tensors behind autograd's back: move their version counters as an in-place op would."""
        tensors = list(tensors)
        if tensors:
            torch._C._autograd._unsafe_set_version_counter(tensors, [t._version + 1 for t in tensors])

    def launch(self, pairs, weight) -> None:
        """ww_weight_average_f32 over `pairs` [(parameter, averaged tensor)], one launch per 16; counts nothing."""
        from . import _native as nat
        from . import ops
        for i in range(0, len(pairs), nat.ADAM_MAX_TENSORS):
            chunk = pairs[i:i + nat.ADAM_MAX_TENSORS]
            key = tuple((p.data_ptr(), a.data_ptr(), p.numel()) for p, a in chunk)
            held = self._tables.get(key)
            if held is None:
                if len(self._tables) > 64:
                    self._tables.clear()
                ps = [p for p, _ in chunk]
                held = self._tables[key] = (ops.adam_table(ps, ps, ps, ps), ops.average_pointers([a for _, a in chunk], ps))
            ops.weight_average_launch(held[0], held[1], chunk[0][0].device, weight)
        self.touched(a for _, a in pairs)

    # ---- on its own ----
    @torch.no_grad()
    def update(self, model=None) -> bool:
        """One update from `model` (default: the model given at construction; another instance of the same class is paired by
        parameter name).  Returns False for an update skipped before `start`."""
        if model is not None and model is not self.source:
            named = dict(model.named_parameters())
            if list(named) != self._names:
                raise ValueError("WeightAverage.update: the model's parameter names differ from the averaged model's")
            pairs = [(named[k], self._avg[k]) for k in self._names]
        else:
            pairs = self.pairs()
        w = self.next_weight()
        if w is not None:
            self.launch(pairs, w)
        self.advance(w is not None)
        return w is not None

    # ---- state ----
    def state_dict(self):
        return {"mode": self.mode, "decay": self.decay, "warmup": self.warmup, "every": self.every, "start": self.start,
                "n_averaged": self.n_averaged, "n_calls": self.n_calls, "parameters": self.model.state_dict()}

    def load_state_dict(self, state) -> None:
        self._configure(state["mode"], state["decay"], state["warmup"], state["every"], state["start"])
        self.model.load_state_dict(state["parameters"])
        self.model.eval()
        self.n_averaged = int(state["n_averaged"])
        self.n_calls = int(state.get("n_calls", self.start + self.n_averaged))

    def to_averaged_model_state_dict(self):
        """The state dict of a torch.optim.swa_utils.AveragedModel around the same model class: `n_averaged` and `module.<key>`."""
        out = OrderedDict(n_averaged=torch.tensor(self.n_averaged, dtype=torch.long))
        for k, v in self.model.state_dict().items():
            out["module." + k] = v
        return out

    def load_averaged_model_state_dict(self, state) -> None:
        """Take the averaged weights and the count of an AveragedModel's state dict (the schedule stays this object's)."""
        inner = OrderedDict((k[len("module."):], v) for k, v in state.items() if k.startswith("module."))
        self.model.load_state_dict(inner)
        self.model.eval()
        self.n_averaged = int(state["n_averaged"])
        self.n_calls = self.start + self.n_averaged
