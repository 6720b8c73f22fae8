"""The class mix of an epoch: `balanced_order`, the one draw behind `positive_fraction=` of both loaders."""
from __future__ import annotations

import numpy as np
import torch


def check_positive_fraction(positive_fraction, shuffle):
    """None, or a float in (0, 1) that needs shuffle=True."""
    if positive_fraction is None:
        return None
    if isinstance(positive_fraction, bool) or not isinstance(positive_fraction, (int, float)) or not 0.0 < float(positive_fraction) < 1.0:
        raise ValueError(f"positive_fraction {positive_fraction!r}: expected None or a number in (0, 1)")
    if not shuffle:
        raise ValueError("positive_fraction: a class-balanced epoch is a random draw; it needs shuffle=True")
    return float(positive_fraction)


def _laid_end_to_end(members: torch.Tensor, count: int) -> torch.Tensor:
    """`count` items of one class: fresh permutations of the class laid end to end and cut, so no item appears more than once more than
    another."""
    m = members.numel()
    perms = [members[torch.randperm(m)] for _ in range((count + m - 1) // m)]
    return torch.cat(perms)[:count]


def balanced_order(labels, positive_fraction) -> torch.Tensor:
    """Item order of one epoch over `labels` (n integers in {0, 1}) that keeps the epoch's length n and fixes its class mix:
    k = min(max(int(positive_fraction n + 0.5), 1), n - 1) positive items and n - k negative ones.  Draws from torch's default generator,
    in this order: the positives' permutations, the negatives' permutations, then one torch.randperm(n) that mixes them --
    `torch.manual_seed` repeats it.  Returns int64 [n]."""
    f = check_positive_fraction(positive_fraction, True)
    if f is None:
        raise ValueError("balanced_order: positive_fraction is None")
    y = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    y = y.reshape(-1)
    if y.size and y.dtype.kind not in "iub":
        raise ValueError("balanced_order: expected integer labels")
    y = y.astype(np.int64)
    if ((y != 0) & (y != 1)).any():
        raise ValueError("balanced_order: a label lies outside {0, 1}")
    pos, neg = torch.from_numpy(np.flatnonzero(y == 1)), torch.from_numpy(np.flatnonzero(y == 0))
    if pos.numel() == 0 or neg.numel() == 0:
        raise ValueError(f"balanced_order: class {1 if pos.numel() == 0 else 0} is missing")
    n = int(y.size)
    k = min(max(int(f * n + 0.5), 1), n - 1)
    picked = torch.cat([_laid_end_to_end(pos, k), _laid_end_to_end(neg, n - k)])
    return picked[torch.randperm(n)]
