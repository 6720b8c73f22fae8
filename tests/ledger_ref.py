"""Restatement of the clip ledger (include/wakeword_amd.h, `ww_clip_ledger_update_f32`) and of every number ledger.LedgerReport derives.

`RefLedger.update` is the per-row contract as a sequential loop over Python integers; the only floating-point steps -- the one float32
subtraction, the clamp, the exact multiply by 2^16 and the round-half-to-even -- are numpy float32 operations, which reproduce the
kernel's Q bit for bit.  `tobytes()` is the device buffer, header included.  The ledger also remembers every scored visit, and the
functions at the bottom recompute the report's quantities from those visits by brute force, in exact rational arithmetic where the
report uses integers."""
import math
from fractions import Fraction

import numpy as np

HEADER_FIELDS = ("n_entries", "updates", "rows", "skipped", "bad_entries", "bad_labels", "nonfinite", "reserved")
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
U64 = 2 ** 64


def margins_q(logits, labels):
    """Per row: (pred, finite, Q) with d = z1 - z0 in float32, pred = z1 > z0, m = d if y == 1 else -d, Q = rint(clamp(m, +-64) * 65536)."""
    z = np.asarray(logits, np.float32).reshape(-1, 2)
    y = np.asarray(labels, np.int64).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        d = z[:, 1] - z[:, 0]                                                  # float32 - float32 -> float32
        pred = (z[:, 1] > z[:, 0]).astype(np.int64)
        m = np.where(y == 1, d, -d).astype(np.float32)
        fin = np.isfinite(m)
        c = np.minimum(np.maximum(np.where(fin, m, np.float32(0)), np.float32(-64)), np.float32(64)) * np.float32(65536)
        assert c.dtype == np.float32
        q = np.rint(c).astype(np.int64)                                        # half to even
    return pred, fin, q


class RefLedger:
    def __init__(self, n_entries):
        self.n_entries = int(n_entries)
        self.header = dict.fromkeys(HEADER_FIELDS, 0)
        self.header["n_entries"] = self.n_entries
        self.recs = [dict(sum_q=0, sum_q2=0, seen_epochs=0, wrong_epochs=0, seen=0, correct=0, nonfinite=0, min_q=INT32_MAX, max_q=INT32_MIN)
                     for _ in range(self.n_entries)]
        self.visits = [[] for _ in range(self.n_entries)]                      # per entry: (epoch, right, Q or None)

    def update(self, logits, labels, entries, epoch):
        labels = np.asarray(labels, np.int64).reshape(-1)
        entries = np.asarray(entries, np.int64).reshape(-1)
        n = labels.size
        assert -1 <= epoch <= 63 and entries.size == n
        if n == 0:
            return
        pred, fin, q = margins_q(logits, labels)
        h = self.header
        h["updates"] += 1
        for i in range(n):
            e, y = int(entries[i]), int(labels[i])
            h["rows"] += 1
            if e < 0:
                h["skipped"] += 1
                continue
            if e >= self.n_entries:
                h["bad_entries"] += 1
                continue
            if y not in (0, 1):
                h["bad_labels"] += 1
                continue
            r = self.recs[e]
            right = int(pred[i]) == y
            r["seen"] += 1
            r["correct"] += int(right)
            if epoch >= 0:
                r["seen_epochs"] |= 1 << epoch
                if not right:
                    r["wrong_epochs"] |= 1 << epoch
            if not fin[i]:
                r["nonfinite"] += 1
                h["nonfinite"] += 1
                self.visits[e].append((epoch, right, None))
                continue
            Q = int(q[i])
            r["sum_q"] += Q
            r["sum_q2"] += Q * Q
            r["min_q"], r["max_q"] = min(r["min_q"], Q), max(r["max_q"], Q)
            self.visits[e].append((epoch, right, Q))

    def tobytes(self) -> bytes:
        out = [np.array([self.header[k] for k in HEADER_FIELDS], "<i8").tobytes()]
        for r in self.recs:
            assert -2 ** 63 <= r["sum_q"] < 2 ** 63 and r["sum_q2"] < U64
            out.append(np.array([r["sum_q"]], "<i8").tobytes())
            out.append(np.array([r["sum_q2"], r["seen_epochs"], r["wrong_epochs"]], "<u8").tobytes())
            out.append(np.array([r["seen"], r["correct"], r["nonfinite"], r["min_q"], r["max_q"], 0], "<i4").tobytes())
        return b"".join(out)


# ---- the report's quantities, by brute force from one entry's visits ------------------------------------------------------------------
def _finite(visits):
    return [q for _, _, q in visits if q is not None]


def mean_margin(visits):
    qs = _finite(visits)
    return float(Fraction(sum(qs), 65536 * len(qs))) if qs else math.nan        # the exact mean, rounded once


def std_margin(visits):
    """The population deviation: the exact rational variance of Q / 65536, then one conversion, one square root."""
    qs = _finite(visits)
    if not qs:
        return math.nan
    mean = Fraction(sum(qs), len(qs))
    var = sum((q - mean) ** 2 for q in qs) / len(qs)
    return math.sqrt(var) / 65536.0


def std_margin_fast(visits):
    """The same number for a long list: Var = E[Q^2] - E[Q]^2 in exact rationals."""
    qs = _finite(visits)
    if not qs:
        return math.nan
    n = len(qs)
    var = Fraction(n * sum(q * q for q in qs) - sum(qs) ** 2, n * n)
    return math.sqrt(var) / 65536.0


def min_margin(visits):
    qs = _finite(visits)
    return min(qs) / 65536.0 if qs else math.nan


def max_margin(visits):
    qs = _finite(visits)
    return max(qs) / 65536.0 if qs else math.nan


def accuracy(visits):
    return sum(int(r) for _, r, _ in visits) / len(visits) if visits else math.nan


def epoch_table(visits):
    """[(epoch, wrong)] over the seen epochs in ascending order; an epoch is wrong when any of its visits was."""
    seen = sorted({ep for ep, _, _ in visits if ep >= 0})
    return [(ep, any(not r for e2, r, _ in visits if e2 == ep)) for ep in seen]


def learned_epoch(visits):
    for ep, wrong in epoch_table(visits):
        if not wrong:
            return ep
    return -1


def forgetting(visits):
    t = epoch_table(visits)
    return sum(1 for (_, w0), (_, w1) in zip(t, t[1:]) if not w0 and w1)


def never_learned(visits):
    t = epoch_table(visits)
    return bool(t) and all(w for _, w in t)


def close(a, b, ulps=4):
    """Equal NaN-ness and within `ulps` units of 2^-53 relative: the report's std_margin rounds when it converts the integer numerator,
    takes the root and divides (three roundings of at most 2^-53 each, the root halving the first); the restatement above rounds the
    rational variance, takes the root and divides.  Four units cover both chains."""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return abs(a - b) <= ulps * 2.0 ** -53 * max(abs(a), abs(b))
