"""FusedAdam: `torch.optim.Adam` whose step is one HIP launch per 16 parameters (csrc/ww_optim.hip, ww_adam_step_f32).

A subclass, not a look-alike: param groups, `state_dict()` / `load_state_dict()` and the state layout (`step`, `exp_avg`, `exp_avg_sq`)
are torch's own, so a state dict moves between this class and `torch.optim.Adam` in both directions, a reference checkpoint's
`optimizer_state_dict` loads, and every torch LR scheduler works (lr, betas, eps and weight_decay are read from the group on every step).
Only the arithmetic of `step()` is replaced; it follows torch's single-tensor Adam operation for operation.

`optimizer.average = WeightAverage(model)` (average.py) keeps an EMA or SWA of the weights inside the same
launches: every launch whose parameters the average covers becomes ww_adam_avg_step_f32, covered parameters that no launch of the step
carried (no gradient) get one stand-alone averaging launch afterwards, and `average.n_averaged` advances once per `step()`.  Only
every="step" averages are fused.  The average is no optimiser state: `state_dict()` is unchanged (the average has its own).

Refused (NotImplementedError at construction): amsgrad, maximize, capturable, differentiable, decoupled_weight_decay, a tensor lr.
Refused (RuntimeError on the step that meets them): parameters or gradients that are not float32, contiguous and on the GPU.
"""
from __future__ import annotations

import torch

from . import _native as nat
from . import ops


class FusedAdam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False, capturable=False,
                 differentiable=False, decoupled_weight_decay=False):
        for name, on in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable), ("differentiable", differentiable),
                         ("decoupled_weight_decay", decoupled_weight_decay)):
            if on:
                raise NotImplementedError(f"FusedAdam: {name}=True is not implemented by the HIP kernel (use torch.optim.Adam)")
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("FusedAdam: a tensor lr is not implemented (the launch takes the value on the host)")
        if not eps > 0.0:
            raise ValueError(f"Invalid epsilon value: {eps} (the kernel divides by sqrt(v) + eps)")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False, fused=False)
        self._tables = {}               # (pointers of a launch's tensors) -> its ctypes table, rebuilt only when a tensor moves
        self.average = None             # average.WeightAverage or None, assignable: see the module text

    @staticmethod
    def _check(p: torch.Tensor, what: str) -> None:
        if p.device.type != "cuda" or p.dtype != torch.float32 or not p.is_contiguous() or p.is_sparse:
            raise RuntimeError(f"FusedAdam: {what} is {p.dtype} on {p.device}, contiguous={p.is_contiguous()}: the kernel takes "
                               "contiguous float32 tensors on the GPU")

    @torch.no_grad()
    def step(self, closure=None, *, grad_scale=None):
        """One update.  `grad_scale`: a float32 [1] GPU tensor every gradient is multiplied by inside the kernel (ops.grad_norm's clip
        scale), read on the device: no host wait."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # an every="step" average rides in the Adam launches (average.WeightAverage); its weight is None while `start` skips updates
        average = self.average if self.average is not None and self.average.every == "step" else None
        avg_weight = None if average is None else average.next_weight()
        fused = set()                                        # id(p) of the parameters an averaged launch carried
        for group in self.param_groups:
            for forbidden in ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay"):
                if group.get(forbidden):
                    raise NotImplementedError(f"FusedAdam: {forbidden}=True is not implemented by the HIP kernel")
            if isinstance(group["lr"], torch.Tensor):
                raise NotImplementedError("FusedAdam: a tensor lr is not implemented")
            by_step = {}                                     # (step count, averaged?) -> [(p, state)]: one launch carries one bias correction
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if len(state) == 0:
                    self._check(p, "a parameter")
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)          # on the host, where torch.optim.Adam keeps it
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                step = state["step"]
                if step.device.type != "cpu":
                    raise RuntimeError("FusedAdam: state['step'] lives on the GPU (a capturable or fused checkpoint); move it to the CPU")
                step += 1
                averaged = avg_weight is not None and average.average_of(p) is not None
                by_step.setdefault((int(step.item()), averaged), []).append((p, state))
            for (t, averaged), entries in by_step.items():
                for i in range(0, len(entries), nat.ADAM_MAX_TENSORS):
                    chunk = entries[i:i + nat.ADAM_MAX_TENSORS]
                    if averaged:
                        self._launch(chunk, group, t, grad_scale, [average.average_of(p) for p, _ in chunk], avg_weight)
                        fused.update(id(p) for p, _ in chunk)
                    else:
                        self._launch(chunk, group, t, grad_scale)
        if average is not None:
            if avg_weight is not None:
                # parameters of the average that no launch of this step carried (no gradient, or not this optimiser's): on their own
                rest = [(p, a) for p, a in average.pairs() if id(p) not in fused]
                if rest:
                    average.launch(rest, avg_weight)
            average.advance(avg_weight is not None)
        return loss

    def _launch(self, entries, group, t, grad_scale, avgs=None, avg_weight=None) -> None:
        key = tuple((p.data_ptr(), p.grad.data_ptr(), s["exp_avg"].data_ptr(), s["exp_avg_sq"].data_ptr(), p.numel()) for p, s in entries)
        if avgs is not None:
            key += tuple(a.data_ptr() for a in avgs)
        table = self._tables.get(key)
        if table is None:
            for p, s in entries:
                self._check(p, "a parameter")
                self._check(p.grad, "a gradient")
            if len(self._tables) > 64:
                self._tables.clear()
            table = ops.adam_table([p for p, _ in entries], [p.grad for p, _ in entries],
                                   [s["exp_avg"] for _, s in entries], [s["exp_avg_sq"] for _, s in entries])
            if avgs is not None:
                table = (table, ops.average_pointers(avgs, [p for p, _ in entries]))
            self._tables[key] = table
        device = entries[0][0].device
        if any(p.device != device for p, _ in entries):
            raise RuntimeError("FusedAdam: the parameters of one group live on different devices")
        if avgs is None:
            ops.adam_launch(table, device, group["lr"], group["betas"], group["eps"], group["weight_decay"], t, grad_scale)
        else:
            ops.adam_average_launch(table[0], table[1], device, group["lr"], group["betas"], group["eps"], group["weight_decay"], t, avg_weight,
                                    grad_scale)
        # the kernel wrote p, exp_avg and exp_avg_sq (and the averages) behind autograd's back: move their version counters as an in-place op
        # would, so that whatever keys on them (the modules' packed inference weights, autograd's saved-tensor check) sees the update
        tensors = [x for p, s in entries for x in (p, s["exp_avg"], s["exp_avg_sq"])] + list(avgs or ())
        torch._C._autograd._unsafe_set_version_counter(tensors, [x._version + 1 for x in tensors])
