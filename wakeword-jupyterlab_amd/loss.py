"""Losses for imbalanced wake-word data: FocalLoss as a plain torch module, sklearn's "balanced" class
weights, and the one place that turns loss options into the values ww_ce_loss_ex_f32 takes.  Host code only: nothing here needs the
native library, so hand-written loops and `inference.evaluate(..., criterion=)` can use FocalLoss on the CPU as well as on the GPU;
WakewordTrainer computes the same loss in its fused step when `trainer.criterion` is set to one.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn

REDUCTIONS = ("mean", "sum")


def check_weight(weight):
    """None or two finite class weights >= 0 (a tensor, on any device, or two numbers) -> None or a tuple of two floats.  A tensor is
    copied to the host here."""
    if weight is None:
        return None
    if isinstance(weight, torch.Tensor):
        if weight.dim() != 1 or weight.numel() != 2:
            raise ValueError(f"weight: expected two class weights, got a tensor of shape {tuple(weight.shape)}")
        weight = weight.detach().cpu().tolist()
    try:
        w = tuple(float(v) for v in weight)
    except TypeError:
        raise ValueError(f"weight: expected two class weights, got {weight!r}") from None
    if len(w) != 2:
        raise ValueError(f"weight: expected two class weights, got {len(w)}")
    if not all(math.isfinite(v) and v >= 0.0 for v in w):
        raise ValueError(f"weight: expected finite values >= 0, got {w}")
    return w


def check_options(weight=None, label_smoothing=0.0, ignore_index=-100, reduction="mean", focal_gamma=None):
    """The loss options as checked host values: (weight or None, label_smoothing, ignore_index, reduction, focal_gamma or None).
    ValueError for a bad value, NotImplementedError for reduction="none"; nothing touches a device except a weight tensor's copy."""
    w = check_weight(weight)
    if isinstance(label_smoothing, bool) or not isinstance(label_smoothing, (int, float)) or not 0.0 <= float(label_smoothing) <= 1.0:
        raise ValueError(f"label_smoothing {label_smoothing!r}: expected a number in [0, 1]")
    if isinstance(ignore_index, bool) or not isinstance(ignore_index, (int, np.integer)) or not -2 ** 63 <= int(ignore_index) < 2 ** 63:
        raise ValueError(f"ignore_index {ignore_index!r}: expected an integer")
    if reduction == "none":
        raise NotImplementedError('reduction="none": the fused loss returns the batch mean or sum ("mean", "sum")')
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction {reduction!r}: expected one of {REDUCTIONS}")
    if focal_gamma is not None:
        if isinstance(focal_gamma, bool) or not isinstance(focal_gamma, (int, float)) or not (math.isfinite(focal_gamma) and focal_gamma >= 0.0):
            raise ValueError(f"focal_gamma {focal_gamma!r}: expected a finite number >= 0 or None")
        if float(label_smoothing) != 0.0:
            raise ValueError("label_smoothing: the focal loss takes none (focal_gamma is given)")
        focal_gamma = float(focal_gamma)
    return w, float(label_smoothing), int(ignore_index), reduction, focal_gamma


class FocalLoss(nn.Module):
    """Focal loss over two classes (Lin et al. 2017, reduced as torchvision's sigmoid_focal_loss is): per clip, with p = softmax(input),
    y the target and q the OTHER class's probability,

        l = weight[y] * q ** gamma * (-log p_y)

    `reduction="mean"` divides the sum by the NUMBER of clips that are not ignored (not by their weights), "sum" by 1, "none" returns
    the clips' losses (an ignored clip's is 0).  gamma = 0 with no weight is cross-entropy.  q ** gamma is taken as
    exp(gamma * log_softmax(input)[other]): q is never formed as 1 - p_y, and the gradient stays finite where q underflows.
    Plain torch, autograd-able, CPU or GPU; `trainer.criterion = FocalLoss(...)` runs it inside the fused step instead."""

    def __init__(self, gamma=2.0, weight=None, reduction="mean", ignore_index=-100):
        super().__init__()
        if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not (math.isfinite(gamma) and gamma >= 0.0):
            raise ValueError(f"gamma {gamma!r}: expected a finite number >= 0")
        if reduction not in REDUCTIONS + ("none",):
            raise ValueError(f"reduction {reduction!r}: expected 'mean', 'sum' or 'none'")
        if isinstance(ignore_index, bool) or not isinstance(ignore_index, (int, np.integer)):
            raise ValueError(f"ignore_index {ignore_index!r}: expected an integer")
        w = check_weight(weight)
        self.gamma, self.reduction, self.ignore_index = float(gamma), reduction, int(ignore_index)
        if w is None:
            self.weight = None
        else:
            self.register_buffer("weight", weight.detach().clone() if isinstance(weight, torch.Tensor) else torch.tensor(w, dtype=torch.float32))

    def extra_repr(self):
        return f"gamma={self.gamma}, reduction={self.reduction!r}, ignore_index={self.ignore_index}"

    def forward(self, input, target):
        if input.dim() != 2 or input.shape[1] != 2:
            raise ValueError(f"FocalLoss: expected logits [n, 2], got {tuple(input.shape)}")
        if target.dim() == 2 and target.shape[1] == 1:
            target = target[:, 0]
        if target.dim() != 1 or target.shape[0] != input.shape[0] or target.dtype != torch.int64:
            raise ValueError(f"FocalLoss: expected int64 targets [{input.shape[0]}], got {target.dtype} {tuple(target.shape)}")
        keep = target != self.ignore_index
        y = torch.where(keep, target, torch.zeros_like(target))
        logp = torch.log_softmax(input, dim=1)
        logp_y = logp.gather(1, y[:, None])[:, 0]
        logq = logp.gather(1, (1 - y)[:, None])[:, 0]
        loss = torch.exp(self.gamma * logq) * -logp_y
        if self.weight is not None:
            loss = loss * self.weight.to(dtype=input.dtype, device=input.device)[y]
        loss = torch.where(keep, loss, torch.zeros_like(loss))
        if self.reduction == "none":
            return loss
        if self.reduction == "sum":
            return loss.sum()
        return loss.sum() / keep.sum().to(loss.dtype)


def check_distillation(alpha=0.5, temperature=2.0):
    """The mixing weight and the temperature of a distillation loss as checked host floats: alpha in [0, 1], a finite temperature > 0.
    ValueError otherwise."""
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"alpha {alpha!r}: expected a number in [0, 1]")
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not (math.isfinite(temperature) and temperature > 0.0):
        raise ValueError(f"temperature {temperature!r}: expected a finite number > 0")
    return float(alpha), float(temperature)


class DistillationLoss(nn.Module):
    """Hinton's knowledge-distillation loss over two classes, with z the student's logits and zt the teacher's:

        L = (1 - alpha) * H(z, target) + alpha * T^2 * KD(z, zt)
        KD = mean over rows of sum_c q_c (log q_c - log p_c),   q = softmax(zt / T),  p = softmax(z / T)

    i.e. F.kl_div(log_softmax(z / T), softmax(zt / T), reduction="batchmean") * T^2.  H is `criterion`: an nn.CrossEntropyLoss (the
    default; weight, label_smoothing, ignore_index, reduction "mean" or "sum") or a FocalLoss.  `target` is int64 labels [n] or [n, 1]
    -- a label equal to ignore_index or outside {0, 1} adds nothing --, float32/float64 class probabilities [n, 2] (a row counts iff
    both entries are finite and >= 0; cross-entropy only, divided by the NUMBER of counted rows), or None: unlabelled audio,
    L = T^2 KD and alpha is not read.  A row counts for KD iff both teacher logits are finite.  Under "mean" each term has its own
    denominator (the criterion's, and the number of KD rows); under "sum" both divide by 1.  A term without a counted row contributes
    exactly 0; when neither has one the loss is NaN and the gradient zero.  No gradient flows to `teacher_logits`.
    Plain torch, autograd-able, CPU or GPU; WakewordTrainer(teacher=...) computes the same loss inside the fused step."""

    def __init__(self, alpha=0.5, temperature=2.0, criterion=None):
        super().__init__()
        self.alpha, self.temperature = check_distillation(alpha, temperature)
        criterion = nn.CrossEntropyLoss() if criterion is None else criterion
        if not isinstance(criterion, FocalLoss) and type(criterion) is not nn.CrossEntropyLoss:
            raise TypeError(f"DistillationLoss: the hard term is nn.CrossEntropyLoss or FocalLoss, not {type(criterion).__name__}")
        if criterion.reduction not in REDUCTIONS:
            raise NotImplementedError('reduction="none": the distillation loss returns the batch mean or sum ("mean", "sum")')
        self.criterion = criterion
        # the focal criterion as a sum over the counted rows (its options are read here, once): the mean's denominator is applied in forward
        self._focal_sum = FocalLoss(criterion.gamma, criterion.weight, "sum") if isinstance(criterion, FocalLoss) else None

    def extra_repr(self):
        return f"alpha={self.alpha}, temperature={self.temperature}"

    def _hard(self, z, target):
        """(sum of the counted rows' losses, the mean's denominator as a 0-d tensor) of the criterion on `target`."""
        crit = self.criterion
        focal = isinstance(crit, FocalLoss)
        w = None if crit.weight is None else crit.weight.to(dtype=z.dtype, device=z.device)
        if target.dtype.is_floating_point:
            if focal:
                raise NotImplementedError("DistillationLoss: class-probability targets with a FocalLoss criterion are not supported")
            if int(crit.ignore_index) != -100:
                raise ValueError(f"ignore_index {crit.ignore_index}: class-probability targets take none")
            if target.shape != z.shape:
                raise ValueError(f"DistillationLoss: expected class probabilities {tuple(z.shape)}, got {tuple(target.shape)}")
            valid = torch.isfinite(target).all(dim=1) & (target >= 0).all(dim=1)
            zv, tv = z[valid], target[valid].to(z.dtype)
            total = nn.functional.cross_entropy(zv, tv, weight=w, label_smoothing=crit.label_smoothing, reduction="sum")
            return total, valid.sum().to(z.dtype)
        if target.dim() == 2 and target.shape[1] == 1:
            target = target[:, 0]
        if target.dim() != 1 or target.shape[0] != z.shape[0] or target.dtype != torch.int64:
            raise ValueError(f"DistillationLoss: expected int64 targets [{z.shape[0]}], got {target.dtype} {tuple(target.shape)}")
        valid = (target != crit.ignore_index) & ((target == 0) | (target == 1))
        zv, yv = z[valid], target[valid]
        if focal:
            return self._focal_sum(zv, yv), valid.sum().to(z.dtype)
        total = nn.functional.cross_entropy(zv, yv, weight=w, label_smoothing=crit.label_smoothing, reduction="sum")
        return total, (valid.sum().to(z.dtype) if w is None else w[yv].sum())

    def forward(self, input, teacher_logits, target=None):
        if input.dim() != 2 or input.shape[1] != 2:
            raise ValueError(f"DistillationLoss: expected logits [n, 2], got {tuple(input.shape)}")
        if teacher_logits.shape != input.shape:
            raise ValueError(f"DistillationLoss: expected teacher logits {tuple(input.shape)}, got {tuple(teacher_logits.shape)}")
        mean = self.criterion.reduction == "mean"
        T = self.temperature
        zt = teacher_logits.detach().to(device=input.device, dtype=input.dtype)
        rows = torch.isfinite(zt).all(dim=1)
        logq, logp = torch.log_softmax(zt[rows] / T, dim=1), torch.log_softmax(input[rows] / T, dim=1)
        kd = (T * T) * (logq.exp() * (logq - logp)).sum()
        kd_denom = rows.sum().to(input.dtype) if mean else torch.ones((), dtype=input.dtype, device=input.device)
        kd_has = bool(kd_denom > 0)
        if target is None:
            hard, hard_has, ch, ck = None, False, 0.0, 1.0
        else:
            hard, hard_denom = self._hard(input, target.to(input.device))
            if not mean:
                hard_denom = torch.ones_like(hard_denom)
            hard_has, ch, ck = bool(hard_denom > 0), 1.0 - self.alpha, self.alpha
        # an exact 0 that hangs on `input` with a gradient of zeros, whatever input holds (0 * inf is never formed)
        loss = torch.where(torch.zeros_like(input, dtype=torch.bool), input, torch.zeros_like(input)).sum()
        if not hard_has and not kd_has:                      # the mean over nothing: NaN, with a gradient of zeros
            return loss + float("nan")
        if hard_has and ch > 0.0:
            loss = loss + ch * (hard / hard_denom)
        if kd_has and ck > 0.0:
            loss = loss + ck * (kd / kd_denom)
        return loss


def balanced_class_weights(labels) -> torch.Tensor:
    """sklearn's class_weight="balanced" for labels over {0, 1}: tensor([n / (2 n0), n / (2 n1)]), float32 -- what
    nn.CrossEntropyLoss(weight=) and FocalLoss(weight=) take.  Both classes must be present."""
    y = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    y = y.reshape(-1)
    if y.size == 0 or y.dtype.kind not in "iub":
        raise ValueError("balanced_class_weights: expected a non-empty array of integer labels")
    y = y.astype(np.int64)
    if ((y != 0) & (y != 1)).any():
        raise ValueError("balanced_class_weights: a label lies outside {0, 1}")
    n1 = int(y.sum())
    n0 = int(y.size) - n1
    if n0 == 0 or n1 == 0:
        raise ValueError(f"balanced_class_weights: class {0 if n0 == 0 else 1} is missing")
    return torch.tensor([y.size / (2.0 * n0), y.size / (2.0 * n1)], dtype=torch.float32)
