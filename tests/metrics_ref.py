"""Restatement of the clip-evaluation counters (include/wakeword_amd.h, `ww_clip_metrics`) and of every number metrics.ClipReport derives
from them, in plain numpy: the counters clip by clip from logits and labels, the report dict and text from per-class counts, the ROC,
AUC and EER from the histogram, and the exact Mann-Whitney AUC of the unbinned margins.  Written from the rules, not from the package's
code: the margins of the operating points are the one thing taken from the library (nobody recomputes them)."""
import numpy as np

BINS = 4096
NAMES = ("Negative", "Wakeword")


def margins_of(logits):
    z = np.asarray(logits, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        return (z[:, 1] - z[:, 0]).astype(np.float32)        # one float32 subtraction


def bins_of(d):
    """bin = clamp(floor((d + 32) * 64), 0, 4095) in float32 arithmetic, for finite d."""
    d = np.asarray(d, np.float32)
    with np.errstate(over="ignore"):
        t = np.floor((d + np.float32(32.0)) * np.float32(64.0))
    assert t.dtype == np.float32
    return np.clip(t, 0.0, float(BINS - 1)).astype(np.int64)


def counters(logits, labels, margins):
    """The record after these clips, one clip at a time."""
    z = np.asarray(logits, np.float32).reshape(-1, 2)
    y = np.asarray(labels, np.int64).reshape(-1)
    m = np.asarray(margins, np.float32).reshape(-1)
    d = margins_of(z)
    out = {"argmax": np.zeros((2, 2), np.int64), "total": len(y), "bad_labels": 0, "nonfinite": 0,
           "at": np.zeros((len(m), 2, 2), np.int64), "hist": np.zeros((2, BINS), np.int64)}
    b = bins_of(np.where(np.isfinite(d), d, np.float32(0)))
    for i in range(len(y)):
        if y[i] not in (0, 1):
            out["bad_labels"] += 1
            continue
        out["argmax"][y[i], 1 if z[i, 1] > z[i, 0] else 0] += 1
        if not np.isfinite(d[i]):
            out["nonfinite"] += 1
            continue
        for k in range(len(m)):
            out["at"][k, y[i], 1 if d[i] >= m[k] else 0] += 1
        out["hist"][y[i], b[i]] += 1
    return out


def assert_counters(report, want, batches=None):
    """Every counter of a ClipReport equals the restatement's, integer for integer."""
    assert np.array_equal(report.confusion, want["argmax"]), (report.confusion, want["argmax"])
    assert report.clips_seen == want["total"] and report.bad_labels == want["bad_labels"] and report.nonfinite == want["nonfinite"]
    assert np.array_equal(report.at_counts, want["at"]), (report.at_counts, want["at"])
    assert np.array_equal(report.hist, want["hist"]), np.nonzero(report.hist != want["hist"])
    if batches is not None:
        assert report.batches == batches


# ---- sklearn's report from a confusion matrix [label][prediction] ----
def _ratio(a, b):
    return float(a) / float(b) if b else 0.0


def report_dict(confusion):
    c = np.asarray(confusion, np.int64)
    out, rows = {}, []
    for k, name in enumerate(NAMES):
        tp, pred, true = int(c[k, k]), int(c[:, k].sum()), int(c[k].sum())
        row = [_ratio(tp, pred), _ratio(tp, true), _ratio(2 * tp, pred + true), true]
        rows.append(row)
        out[name] = {"precision": row[0], "recall": row[1], "f1-score": row[2], "support": float(true)}
    n = int(c.sum())
    out["accuracy"] = _ratio(int(c[0, 0] + c[1, 1]), n)
    out["macro avg"] = {h: (rows[0][j] + rows[1][j]) / 2.0 for j, h in enumerate(("precision", "recall", "f1-score"))}
    out["weighted avg"] = {h: _ratio(rows[0][j] * rows[0][3] + rows[1][j] * rows[1][3], n) for j, h in enumerate(("precision", "recall", "f1-score"))}
    out["macro avg"]["support"] = out["weighted avg"]["support"] = float(n)
    return out


def report_text(confusion):
    r = report_dict(confusion)
    lines = ["%12s  %9s %9s %9s %9s" % ("", "precision", "recall", "f1-score", "support"), ""]
    for name in NAMES + ("", "accuracy", "macro avg", "weighted avg"):
        if name == "":
            lines.append("")
        elif name == "accuracy":
            lines.append("%12s  %9s %9s %9.2f %9d" % (name, "", "", r["accuracy"], r["macro avg"]["support"]))
        else:
            v = r[name]
            lines.append("%12s  %9.2f %9.2f %9.2f %9d" % (name, v["precision"], v["recall"], v["f1-score"], v["support"]))
    return "\n".join(lines) + "\n"


# ---- the curve from the histogram ----
def roc(hist):
    """fpr, tpr at the 4097 edges: at edge j the clips in bins >= j fire."""
    h = np.asarray(hist, np.float64)
    fpr, tpr = np.zeros(BINS + 1), np.zeros(BINS + 1)
    neg, pos = h[0].sum(), h[1].sum()
    for j in range(BINS + 1):
        fpr[j] = h[0, j:].sum() / neg if neg else 0.0
        tpr[j] = h[1, j:].sum() / pos if pos else 0.0
    return fpr, tpr


def auc_binned(hist):
    """Mann-Whitney on the bin indices: P(bin of a positive > bin of a negative) + P(equal) / 2."""
    h = np.asarray(hist, np.float64)
    below = np.concatenate([[0.0], np.cumsum(h[0])[:-1]])
    return float(np.sum(h[1] * (below + 0.5 * h[0])) / (h[0].sum() * h[1].sum()))


def auc_exact(d, y):
    """Mann-Whitney on the finite margins themselves, ties one half."""
    d, y = np.asarray(d, np.float64), np.asarray(y)
    keep = np.isfinite(d) & ((y == 0) | (y == 1))
    neg, pos = np.sort(d[keep & (y == 0)]), d[keep & (y == 1)]
    lo, hi = np.searchsorted(neg, pos, "left"), np.searchsorted(neg, pos, "right")
    return float(np.sum(lo + 0.5 * (hi - lo)) / (len(neg) * len(pos)))


def auc_bound(hist):
    h = np.asarray(hist, np.float64)
    return float(np.sum(h[0] * h[1]) / (2.0 * h[0].sum() * h[1].sum()))


def eer(hist):
    """Between the last edge with fpr >= fnr and the next, both rates run linearly; the EER is where they meet."""
    fpr, tpr = roc(hist)
    fnr = 1.0 - tpr
    for j in range(BINS):
        if fpr[j] >= fnr[j] and fpr[j + 1] < fnr[j + 1]:
            last = j
    a, b = fpr[last] - fnr[last], fpr[last + 1] - fnr[last + 1]
    t = a / (a - b)
    return float(fpr[last] + t * (fpr[last + 1] - fpr[last]))
