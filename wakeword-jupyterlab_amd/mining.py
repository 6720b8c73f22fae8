"""Online hard example mining: which rows of a candidate batch the fused training step trains on.

`HardSelect(keep, keep_class=None)` is a rule, not a buffer: `WakewordTrainer(..., select=HardSelect(0.25, keep_class=1))` scores every
batch with a dropout-free forward, ranks the rows by the criterion's own per-clip loss on the device (ops.hard_select_into) and runs the
step on the `rows(B)` hardest.  Pure host code; the kernels are in csrc/ww_select.hip."""
from __future__ import annotations

import math
import numbers


class HardSelect:
    """keep        an integer: that many rows of every batch (a batch of fewer rows is kept whole); or a float in (0, 1]: that fraction
                   of the batch, rounded up, at least one row.  A bool, a float outside (0, 1] or an integer < 1 is refused here.
       keep_class  None, or 0 / 1: counting rows of this class are taken first, whatever their loss (keep every positive, mine the
                   negatives), and the rest of `keep` is filled with the hardest other rows."""

    def __init__(self, keep, keep_class=None):
        if isinstance(keep, bool) or not isinstance(keep, numbers.Real):
            raise TypeError(f"HardSelect: keep must be an integer (rows) or a float in (0, 1] (a fraction), got {type(keep).__name__}")
        if isinstance(keep, numbers.Integral):
            keep = int(keep)
            if keep < 1:
                raise ValueError(f"HardSelect: keep {keep}: expected at least 1 row")
        else:
            keep = float(keep)
            if not 0.0 < keep <= 1.0:                         # NaN fails both comparisons
                raise ValueError(f"HardSelect: keep {keep}: a fraction lies in (0, 1]")
        if keep_class is not None:
            if isinstance(keep_class, bool) or not isinstance(keep_class, numbers.Integral):
                raise TypeError(f"HardSelect: keep_class must be None, 0 or 1, got {type(keep_class).__name__}")
            keep_class = int(keep_class)
            if keep_class not in (0, 1):
                raise ValueError(f"HardSelect: keep_class {keep_class}: expected None, 0 or 1")
        self.keep = keep
        self.keep_class = keep_class

    def rows(self, B: int) -> int:
        """The rows kept of a batch of B: min(keep, B) for a count, max(1, ceil(keep * B)) for a fraction."""
        B = int(B)
        if B < 1:
            raise ValueError(f"HardSelect.rows: a batch of {B} rows")
        if isinstance(self.keep, int):
            return min(self.keep, B)
        return min(B, max(1, math.ceil(round(self.keep * B, 9))))      # 0.3 * 10 is 3.0000000000000004: 3 rows, not 4

    def __repr__(self):
        return f"HardSelect(keep={self.keep!r}, keep_class={self.keep_class!r})"
