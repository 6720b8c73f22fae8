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
