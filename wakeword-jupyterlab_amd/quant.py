"""WeightQuant: int8 post-training quantisation of a model's weights on the GPU, a fake-quant model and an export.

The workflow ends on a model that fits a small device, and a small device stores int8 weights.  This module turns the float32 weights
into them without leaving the GPU, says what that costs, and writes a file both sides can read:

  ops.quantize_weights        the kernel alone (ww_quant_weights_f32): symmetric, `bits` in 2..8, one scale per output channel / row or
                              per tensor; q, scale, the dequantised weights and the error sums in one launch per 16 tensors
  WeightQuant(model)          .model is a module of the model's own class whose weights ARE the dequantised tensors -- a fake-quant
                              model that forward, forward_pcm, evaluate_report, scan_files, det_curve, StreamingDetector and
                              save_deployment_package take as they take any model; .update() re-quantises, .report() says what it cost
  save_quantized_package      the reference's deployment dict with the dequantised float32 weights, plus a "quantized" entry (q, scale)
  load_quantized_package      rebuilds the weights from q * scale alone, on the CPU or the GPU: the bits of WeightQuant.model
  WakewordTrainer(quant=, evaluate="quant")   validation, the monitor and the best checkpoint follow the quantised model

  WeightQuant(clip="mse")     a clipped scale per row: of 48 candidates amax * (64 - j) / 64 the one with the smallest squared error
                              (ww_quant_clip_search_f32 at .calibrate(), ww_quant_weights_clip_f32 at every .update()); section 3t
  WakewordTrainer(quant=, qat=True)           quantisation-aware training: the step's forward and backward read the fake-quant weights,
                              the gradients of clipped weights are cut (ww_quant_ste_f32), Adam moves the float32 master weights

The arithmetic has one definition (include/wakeword_amd.h); tests/quant_ref.py and tests/qat_ref.py restate it in numpy.  Out of scope:
activation quantisation, int8 forward kernels, learned step sizes -- the fake-quant model runs the float32 kernels on int8-representable
weights.
"""
from __future__ import annotations

import copy
import math
from collections import OrderedDict

import torch


class QuantReport:
    """What a quantisation cost, per tensor and in total.

    .tensors   [dict] per quantised tensor: name, shape, rows, cols, fp32_bytes, int8_bytes (the int8 values and the float32 scales),
               sqnr_db (10 log10 of sum w^2 / sum (w - deq)^2 from the kernel's float64 sums: inf when nothing was lost, nan for an
               all-zero tensor), max_error (the largest |w - deq|), nonfinite (elements that were NaN or +-Inf: they quantise to 0)
    .totals    the same over all quantised tensors, plus float_bytes: what stayed float32 (the biases, by default)
    .clip      "max" or "mse"; under "mse" every tensor also has saturated (elements the clamp moved) and clip_min / clip_mean (the
               smallest and the mean clip fraction of its rows; 1.0 is the unclipped scale), and the totals the same
    str()      a table"""

    def __init__(self, bits, per_channel, tensors, float_bytes, clip="max"):
        self.bits, self.per_channel, self.tensors, self.clip = bits, per_channel, tensors, clip
        sw, se = sum(t["sum_w2"] for t in tensors), sum(t["sum_err2"] for t in tensors)
        self.totals = {"tensors": len(tensors), "rows": sum(t["rows"] for t in tensors),
                       "fp32_bytes": sum(t["fp32_bytes"] for t in tensors), "int8_bytes": sum(t["int8_bytes"] for t in tensors),
                       "float_bytes": float_bytes, "sum_w2": sw, "sum_err2": se, "sqnr_db": sqnr_db(sw, se),
                       "max_error": max([t["max_error"] for t in tensors], default=0.0), "nonfinite": sum(t["nonfinite"] for t in tensors)}
        if clip == "mse":
            rows = max(1, self.totals["rows"])
            self.totals.update(saturated=sum(t["saturated"] for t in tensors), clip_min=min([t["clip_min"] for t in tensors], default=1.0),
                               clip_mean=sum(t["clip_mean"] * t["rows"] for t in tensors) / rows)

    def __str__(self):
        mse = self.clip == "mse"
        head = f"{'tensor':<22}{'shape':<20}{'rows':>6}{'fp32 B':>10}{'int8 B':>10}{'SQNR dB':>10}{'max err':>12}{'non-finite':>12}"
        if mse:
            head += f"{'saturated':>11}{'clip min':>10}{'clip mean':>11}"
        title = f"int{self.bits} weights, {'one scale per row' if self.per_channel else 'one scale per tensor'}"
        lines = [title + (", clipped to the smallest squared error" if mse else ""), head, "-" * len(head)]
        for t in self.tensors + [dict(self.totals, name="total", shape="")]:
            shape = "x".join(str(s) for s in t["shape"]) if t["shape"] != "" else ""
            lines.append(f"{t['name']:<22}{shape:<20}{t['rows']:>6}{t['fp32_bytes']:>10}{t['int8_bytes']:>10}{t['sqnr_db']:>10.2f}"
                         f"{t['max_error']:>12.3e}{t['nonfinite']:>12}"
                         + (f"{t['saturated']:>11}{t['clip_min']:>10.4f}{t['clip_mean']:>11.4f}" if mse else ""))
        lines.append(f"kept in float32: {self.totals['float_bytes']} bytes")
        return "\n".join(lines)


def sqnr_db(sum_w2: float, sum_err2: float) -> float:
    """10 log10(sum w^2 / sum err^2): inf when the error is zero, nan when the signal is."""
    if not sum_w2 > 0.0:
        return float("nan")
    if not sum_err2 > 0.0:
        return float("inf")
    return 10.0 * math.log10(sum_w2 / sum_err2)


def dequantize(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """float32(q) * scale with one scale per slice of q's first dimension (scale [rows]) or one for the tensor (scale [1]): ONE float32
    multiplication per element, on whatever device q is.  This is the kernel's deq, bit for bit."""
    if q.dtype != torch.int8 or scale.dtype != torch.float32:
        raise TypeError(f"dequantize: expected int8 values and float32 scales, got {q.dtype} and {scale.dtype}")
    rows = scale.numel()
    if rows != 1 and (q.dim() < 2 or q.shape[0] != rows):
        raise ValueError(f"dequantize: {rows} scales for values of shape {tuple(q.shape)}")
    return q.to(torch.float32) * scale.reshape((rows,) + (1,) * (q.dim() - 1) if rows != 1 else (1,) * q.dim())


def _check_options(bits, per_channel, quantize_bias, clip="max"):
    from .ops import check_quant_bits, check_quant_clip
    bits = check_quant_bits(bits)
    for name, v in (("per_channel", per_channel), ("quantize_bias", quantize_bias)):
        if not isinstance(v, bool):
            raise TypeError(f"{name} {v!r}: expected a bool")
    check_quant_clip(clip)
    return bits, per_channel, quantize_bias


def clip_fractions(clip: torch.Tensor) -> torch.Tensor:
    """The fractions (64 - j) / 64 of clip indices j (an index past the last candidate counts as the last), float32, exact."""
    from ._native import QUANT_CLIP_STEPS
    return (64.0 - clip.to(torch.float32).clamp(max=QUANT_CLIP_STEPS - 1)) / 64.0


class WeightQuant:
    """The quantised weights of `model` (a SimpleWakewordModel or a WakewordModel; `average.model` is one).

    .model        a module of the model's own class in eval mode, without gradients, on the model's device.  Its weight parameters are
                  the kernel's dequantised output, so every evaluator of the package takes it as a model; parameters with one dimension
                  (the biases) are float32 copies unless `quantize_bias`, which quantises them with one scale per tensor.
    .update()     re-quantises from the source's current weights: one launch per 16 tensors, no wait, no allocation after the first call;
                  the written tensors' version counters move as for an in-place op, so `.model.packed_weights()` rebuilds
    .report()     a QuantReport, from ONE device-to-host copy
    .q, .scale    {parameter name: int8 tensor of the weight's shape} and {name: float32 [rows]}

    clip="max" (the default) takes every row's scale from its largest element.  clip="mse" gives up a row's outliers for a finer step:
    .clip         {name: uint8 [rows]} the row's candidate index j; its scale is max(amax * ((64 - j) / 64) / qmax, 2^-126).  Empty under "max".
    .calibrate()  searches every row's 48 candidates for the smallest squared error (one launch per 16 tensors, no wait), then update().
                  Construction on the GPU calibrates once; update() keeps the stored indices and runs no search.

    A model on the GPU is quantised at construction.  Around a model on the CPU the object can be built, load a state dict and write a
    package; update() needs the GPU (there is no CPU implementation of the kernel)."""

    def __init__(self, model, bits=8, per_channel=True, quantize_bias=False, clip="max"):
        from .model import SimpleWakewordModel, WakewordModel
        if not isinstance(model, (SimpleWakewordModel, WakewordModel)):
            raise TypeError(f"WeightQuant: expected a SimpleWakewordModel or a WakewordModel, got {type(model).__name__}")
        self.bits, self.per_channel, self.quantize_bias = _check_options(bits, per_channel, quantize_bias, clip)
        self.clip_mode = clip
        self.source = model
        self.model = copy.deepcopy(model)
        self.model.eval()
        self.model._packed = self.model._packed_key = None                       # the copy packs its own weights on first use
        for p in self.model.parameters():
            p.requires_grad_(False)
            p.grad = None
        self._own = dict(self.model.named_parameters())
        self._names = list(self._own)
        self._allocate()
        self._tables = {}                                    # (pointers of the source's tensors) -> the ctypes tables of an update
        self.n_updates = self.n_calibrations = 0
        if self._device.type == "cuda":
            if self.clip_mode == "mse":
                self.calibrate()
            else:
                self.update()

    # ---- buffers: allocated once ----
    def _groups(self, name):
        """(rows, cols, per-channel?) of a quantised parameter."""
        from .ops import quant_groups
        p = self._own[name]
        mode = self.per_channel and p.dim() >= 2
        return quant_groups(p, mode) + (mode,)

    def _allocate(self):
        """q per tensor, and ONE buffer behind every err, scale and bad -- under clip="mse" also behind every sat and clip, after them
        -- so that report() reads them in one copy."""
        self._device = next(iter(self._own.values())).device
        self.quantized = [k for k in self._names if self._own[k].dim() >= 2 or self.quantize_bias]
        self.kept = [k for k in self._names if k not in self.quantized]
        rows = [self._groups(k)[0] for k in self.quantized]
        total = sum(rows)
        mse = self.clip_mode == "mse"
        self._stats = torch.zeros(total * (24 + 4 + 4 + (4 + 1 if mse else 0)), device=self._device, dtype=torch.uint8)
        err = self._stats[:24 * total].view(torch.float64).view(total, 3)
        scale = self._stats[24 * total:28 * total].view(torch.float32)
        bad = self._stats[28 * total:32 * total].view(torch.int32)
        sat = self._stats[32 * total:36 * total].view(torch.int32) if mse else None
        clip = self._stats[36 * total:] if mse else None
        self.q, self.scale, self._err, self._bad = OrderedDict(), OrderedDict(), OrderedDict(), OrderedDict()
        self.clip, self._sat = OrderedDict(), OrderedDict()
        at = 0
        for k, r in zip(self.quantized, rows):
            self.q[k] = torch.zeros(self._own[k].shape, device=self._device, dtype=torch.int8)
            self.scale[k], self._err[k], self._bad[k] = scale[at:at + r], err[at:at + r], bad[at:at + r]
            if mse:
                self.clip[k], self._sat[k] = clip[at:at + r], sat[at:at + r]
            at += r

    # ---- the update ----
    def _pair(self, model):
        if model is None or model is self.source:
            named = dict(self.source.named_parameters())
        else:
            named = dict(model.named_parameters())
        if list(named) != self._names:
            raise ValueError("WeightQuant.update: the model's parameter names differ from the quantised model's")
        for k in self._names:
            if named[k].shape != self._own[k].shape:
                raise ValueError(f"WeightQuant.update: {k} has shape {tuple(named[k].shape)}, expected {tuple(self._own[k].shape)}")
        return named

    def _tables_of(self, named, search=False):
        """The ctypes tables of an update (or of a search) from these source tensors: built once per set of pointers."""
        from . import _native as nat
        from . import ops
        srcs = [named[k] for k in self.quantized]
        key = (search,) + tuple(s.data_ptr() for s in srcs)
        tables = self._tables.get(key)
        if tables is None:
            if len(self._tables) > 64:
                self._tables.clear()
            tables, step = [], nat.QUANT_MAX_TENSORS
            for i in range(0, len(srcs), step):
                ks = self.quantized[i:i + step]
                col = lambda d: [d[k] for k in ks]                                      # noqa: E731
                modes = [self._groups(k)[2] for k in ks]
                if search:
                    tables.append(ops.quant_clip_table(srcs[i:i + step], col(self.scale), col(self.clip), per_channel=modes))
                elif self.clip_mode == "mse":
                    tables.append(ops.quant_clip_table(srcs[i:i + step], col(self.scale), col(self.clip), col(self.q), col(self._own), col(self._err),
                                                       col(self._bad), col(self._sat), per_channel=modes))
                else:
                    tables.append(ops.quant_table(srcs[i:i + step], col(self.scale), col(self.q), col(self._own), col(self._err), col(self._bad),
                                                  per_channel=modes))
            self._tables[key] = tables
        return tables

    @torch.no_grad()
    def update(self, model=None, weights_only=False) -> None:
        """Quantise the current weights of `model` (default: the model given at construction; another instance of the same class is
        paired by parameter name) into .q, .scale and the parameters of .model.  `weights_only` leaves the kept float32 parameters (the
        biases) of .model as they are: the launch and the version counters alone -- what a QAT step runs, which reads the biases elsewhere."""
        from . import ops
        from .average import WeightAverage
        named = self._pair(model)
        if self._device.type != "cuda":
            raise RuntimeError("WeightQuant.update: the model is on the CPU; this path has no CPU implementation (model.to('cuda'))")
        launch = ops.quantize_weights_clip_launch if self.clip_mode == "mse" else ops.quantize_weights_launch
        for tab in self._tables_of(named):
            launch(tab, self._device, self.bits)
        WeightAverage.touched(self._own[k] for k in self.quantized)     # written behind autograd's back: move the version counters
        if not weights_only:
            for k in self.kept:
                self._own[k].copy_(named[k])                 # float32 as they are; copy_ moves the version counter itself
        self.n_updates += 1

    @torch.no_grad()
    def calibrate(self, model=None) -> None:
        """clip="mse": choose every row's clip index anew from the current weights of `model` -- the candidate with the smallest squared
        error, ww_quant_clip_search_f32, one launch per 16 tensors and no wait -- then update(model).  Under clip="max" it is update(model)."""
        from . import ops
        if self.clip_mode == "mse":
            named = self._pair(model)
            if self._device.type != "cuda":
                raise RuntimeError("WeightQuant.calibrate: the model is on the CPU; this path has no CPU implementation (model.to('cuda'))")
            for tab in self._tables_of(named, search=True):
                ops.quant_clip_search_launch(tab, self._device, self.bits)
            self.n_calibrations += 1
        self.update(model)

    def ste_tables(self, grads: dict, model=None):
        """The ctypes tables of ww_quant_ste_f32 over the quantised tensors: the source's weights, the stored scales and `grads`
        {parameter name: gradient tensor}.  WakewordTrainer(qat=True) launches them after its backward."""
        from . import _native as nat
        from . import ops
        named = self._pair(model)
        step = nat.QUANT_MAX_TENSORS
        return [ops.quant_ste_table([named[k] for k in ks], [self.scale[k] for k in ks], [grads[k] for k in ks],
                                    per_channel=[self._groups(k)[2] for k in ks])
                for ks in (self.quantized[i:i + step] for i in range(0, len(self.quantized), step))]

    # ---- what it cost ----
    def report(self) -> QuantReport:
        host = self._stats.cpu()                             # the one copy
        total = sum(self._groups(k)[0] for k in self.quantized)
        err = host[:24 * total].view(torch.float64).view(total, 3).numpy()
        bad = host[28 * total:32 * total].view(torch.int32).numpy()
        mse = self.clip_mode == "mse"
        if mse:
            sat = host[32 * total:36 * total].view(torch.int32).numpy()
            fraction = clip_fractions(host[36 * total:]).numpy()
        tensors, at = [], 0
        for k in self.quantized:
            rows, cols, _ = self._groups(k)
            e, b = err[at:at + rows], bad[at:at + rows]
            sw, se = float(e[:, 0].sum()), float(e[:, 1].sum())
            tensors.append({"name": k, "shape": tuple(self._own[k].shape), "rows": rows, "cols": cols, "fp32_bytes": 4 * rows * cols,
                            "int8_bytes": rows * cols + 4 * rows, "sum_w2": sw, "sum_err2": se, "sqnr_db": sqnr_db(sw, se),
                            "max_error": float(e[:, 2].max()), "nonfinite": int(b.sum())})
            if mse:
                f = fraction[at:at + rows]
                tensors[-1].update(saturated=int(sat[at:at + rows].sum()), clip_min=float(f.min()), clip_mean=float(f.mean()))
            at += rows
        return QuantReport(self.bits, self.per_channel, tensors, sum(4 * self._own[k].numel() for k in self.kept), self.clip_mode)

    # ---- state ----
    def state_dict(self):
        """bits, per_channel, quantize_bias, q {name: int8}, scale {name: float32 [rows]} and float {name: float32}: the parameters that
        were not quantised.  q * scale and `float` together are .model's weights.  Under clip="mse" also clip {name: uint8 [rows]}: the
        indices the scales were taken at (the scales already hold them; a loader needs q and scale alone)."""
        state = {"bits": self.bits, "per_channel": self.per_channel, "quantize_bias": self.quantize_bias,
                 "q": OrderedDict((k, v.detach().clone()) for k, v in self.q.items()),
                 "scale": OrderedDict((k, v.detach().clone()) for k, v in self.scale.items()),
                 "float": OrderedDict((k, self._own[k].detach().clone()) for k in self.kept)}
        if self.clip_mode == "mse":
            state["clip"] = OrderedDict((k, v.detach().clone()) for k, v in self.clip.items())
        return state

    @torch.no_grad()
    def load_state_dict(self, state) -> None:
        clip_mode = "mse" if "clip" in state else "max"
        bits, per_channel, quantize_bias = _check_options(int(state["bits"]), bool(state["per_channel"]), bool(state.get("quantize_bias", False)),
                                                          clip_mode)
        if (per_channel, quantize_bias, clip_mode) != (self.per_channel, self.quantize_bias, self.clip_mode):
            self.per_channel, self.quantize_bias, self.clip_mode = per_channel, quantize_bias, clip_mode
            self._allocate()
            self._tables = {}
        self.bits = bits
        if list(state["q"]) != self.quantized or list(state["scale"]) != self.quantized or list(state["float"]) != self.kept:
            raise ValueError("WeightQuant.load_state_dict: the state's tensor names differ from the quantised model's")
        if clip_mode == "mse":
            if list(state["clip"]) != self.quantized:
                raise ValueError("WeightQuant.load_state_dict: the state's clip names differ from the quantised model's")
            for k in self.quantized:
                c = state["clip"][k]
                if c.dtype != torch.uint8 or c.numel() != self.clip[k].numel():
                    raise ValueError(f"WeightQuant.load_state_dict: {k}: clip {c.dtype} with {c.numel()} rows, expected uint8 with {self.clip[k].numel()}")
                self.clip[k].copy_(c.reshape(-1))
        for k in self.quantized:
            q, s = state["q"][k], state["scale"][k]
            if q.shape != self.q[k].shape or s.numel() != self.scale[k].numel():
                raise ValueError(f"WeightQuant.load_state_dict: {k}: q {tuple(q.shape)} with {s.numel()} scales, expected "
                                 f"{tuple(self.q[k].shape)} with {self.scale[k].numel()}")
            self.q[k].copy_(q)
            self.scale[k].copy_(s.reshape(-1))
            self._own[k].copy_(dequantize(self.q[k], self.scale[k]))
        for k in self.kept:
            self._own[k].copy_(state["float"][k])
        self.model.eval()


def _to_cpu(obj):
    if isinstance(obj, torch.Tensor):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        return type(obj)((k, _to_cpu(v)) for k, v in obj.items())
    return obj


def save_quantized_package(quant: WeightQuant, path: str, best_val_accuracy=0, epoch=0, device="cuda"):
    """The reference's deployment dict (model.save_deployment_package) of `quant.model` -- so `model_state_dict` holds the DEQUANTISED
    float32 weights and the reference's loader and `load_checkpoint` take the file -- with one more entry, "quantized":
    quant.state_dict() on the CPU.  Returns the dict."""
    from .model import save_deployment_package
    if not isinstance(quant, WeightQuant):
        raise TypeError(f"save_quantized_package: expected a WeightQuant, got {type(quant).__name__}")
    pkg = save_deployment_package(quant.model, path, best_val_accuracy, epoch, device)
    pkg["quantized"] = _to_cpu(quant.state_dict())
    torch.save(pkg, path)
    return pkg


def load_quantized_package(path: str, model, map_location="cpu"):
    """Load a file of save_quantized_package into `model` (on the CPU or the GPU) from its "quantized" entry ALONE: every quantised
    weight is float32(q) * scale, one float32 multiplication in torch, which is the kernel's own last step -- the model gets the bits of
    WeightQuant.model; `model_state_dict` is not read.  `weights_only=True`: nothing in the file runs.  Returns the dict."""
    pkg = torch.load(path, map_location=map_location, weights_only=True)
    if not isinstance(pkg, dict) or "quantized" not in pkg:
        raise ValueError(f"{path}: no 'quantized' entry (a file of save_deployment_package loads with load_checkpoint)")
    state = pkg["quantized"]
    weights = OrderedDict((k, dequantize(q, state["scale"][k])) for k, q in state["q"].items())
    weights.update(state["float"])
    own = model.state_dict()
    if set(weights) != set(own):
        raise ValueError(f"{path}: the quantised tensors' names differ from the model's")
    model.load_state_dict(OrderedDict((k, weights[k]) for k in own))
    return pkg
