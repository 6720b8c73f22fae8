"""ClipReport: every number of the reference's evaluation cell (notebook cell 17) and a ROC curve, from integer counters.

The counters are what `ww_clip_metrics_update_f32` keeps in device memory (include/wakeword_amd.h) and
`ops.read_clip_metrics` copies to the host once; this module is pure numpy -- no torch, no GPU, no sklearn -- so a report can be built
from counts on any host (`ClipReport.from_counts`), merged across loaders or ranks (`a + b`) and printed as sklearn prints it:

  confusion [[tn, fp], [fn, tp]]   at argmax (prediction 1 iff z1 > z0), sklearn's `confusion_matrix` layout
  at[k] [[tn, fp], [fn, tp]]       at the k-th configured operating point: a clip fires iff its margin d = z1 - z0 >= margins[k]
  hist [2][4096]                   per label, the clips' margins in bins 1/64 wide over [-32, 32) (the end bins take the rest)

The ROC curve has one point per bin edge: at edge j (margin -32 + j / 64) a clip counts as fired iff its bin is >= j, so the points
are suffix sums of the histogram.  The score behind the curve is the bin index: AUC, EER and `threshold_for` are those of the binned
margins, and `auc_bound` says how far binning can have moved the AUC.
"""
from __future__ import annotations

import numpy as np

BINS = 4096
BIN_LOW = -32.0
BINS_PER_UNIT = 64.0
MAX_THRESHOLDS = 8
_HEADERS = ("precision", "recall", "f1-score", "support")


def _div(num, den):
    """num / den in float64 with sklearn's default for an undefined ratio: 0.0."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    out = np.zeros(np.broadcast(num, den).shape, np.float64)
    np.divide(num, den, out=out, where=den != 0)
    return out


def _prf(confusion):
    """Per-class precision, recall, F1 and support of a 2 x 2 confusion matrix [label][prediction], as precision_recall_fscore_support."""
    c = np.asarray(confusion, np.int64)
    tp = np.diag(c)
    pred, true = c.sum(axis=0), c.sum(axis=1)
    return _div(tp, pred), _div(tp, true), _div(2 * tp, true + pred), true


def bin_edges():
    """The 4097 margins -32, -32 + 1/64, ..., 32 (exact in float32 and float64)."""
    return BIN_LOW + np.arange(BINS + 1, dtype=np.float64) / BINS_PER_UNIT


def probability_of_margin(margin):
    """softmax(z)[1] of a margin z1 - z0, in float64: 1 / (1 + exp(-margin))."""
    m = np.asarray(margin, np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-m))


class ClipReport:
    """The counters of one evaluation and every number derived from them.  Build with `from_counts` or `ops.read_clip_metrics`."""

    def __init__(self, confusion, hist, margins, at, bad_labels, nonfinite, thresholds=None):
        self.confusion = confusion
        self.hist = hist
        self.margins = margins
        self.at_counts = at
        self.bad_labels = bad_labels
        self.nonfinite = nonfinite
        self.thresholds = thresholds          # the probabilities the margins were made from, where known (ops.new_clip_metrics)
        self.clips_seen = int(confusion.sum()) + bad_labels      # the record's `total`: bad labels included
        self.batches = None                   # the record's `batches` (ops.read_clip_metrics); None for a report built from counts

    @classmethod
    def from_counts(cls, confusion, hist=None, margins=(), at=None, bad_labels=0, nonfinite=0, thresholds=None):
        """confusion [[tn, fp], [fn, tp]]; hist [2][4096] or None (no ROC); margins: the float32 margins of the operating points, as the
        library gives them (`ww_clip_metrics_margin_host`), with at [len(margins)][2][2] as [label][fired]."""
        c = np.array(confusion)
        if c.shape != (2, 2) or not np.issubdtype(c.dtype, np.integer) or (c < 0).any():
            raise ValueError(f"confusion: expected 2 x 2 non-negative integers [[tn, fp], [fn, tp]], got {confusion!r}")
        c = c.astype(np.int64)
        if hist is not None:
            h = np.array(hist)
            if h.shape != (2, BINS) or not np.issubdtype(h.dtype, np.integer) or (h < 0).any():
                raise ValueError(f"hist: expected [2][{BINS}] non-negative integers")
            hist = h.astype(np.int64)
        m = np.array(margins, dtype=np.float32).reshape(-1)
        if m.size > MAX_THRESHOLDS or not np.isfinite(m).all():
            raise ValueError(f"margins: expected at most {MAX_THRESHOLDS} finite values")
        a = np.zeros((0, 2, 2), np.int64) if at is None else np.array(at)
        if a.shape != (m.size, 2, 2) or not np.issubdtype(a.dtype, np.integer) or (a < 0).any():
            raise ValueError(f"at: expected [{m.size}][2][2] non-negative integers, one [label][fired] table per margin")
        if thresholds is not None:
            thresholds = tuple(float(p) for p in thresholds)
            if len(thresholds) != m.size:
                raise ValueError("thresholds: one probability per margin")
        if int(bad_labels) < 0 or int(nonfinite) < 0:
            raise ValueError("bad_labels / nonfinite: expected counts >= 0")
        return cls(c, hist, m, a.astype(np.int64), int(bad_labels), int(nonfinite), thresholds)

    # ---- the argmax numbers: cell 17 ----
    @property
    def support(self):
        return self.confusion.sum(axis=1)

    @property
    def total(self) -> int:
        return int(self.confusion.sum())

    @property
    def accuracy(self) -> float:
        return float(_div(np.trace(self.confusion), self.confusion.sum()))

    def _averages(self):
        p, r, f, s = _prf(self.confusion)
        rows = {"macro avg": [float(np.mean(x)) for x in (p, r, f)]}
        w = s.astype(np.float64)
        rows["weighted avg"] = [float(_div((x * w).sum(), w.sum())) for x in (p, r, f)]
        return p, r, f, s, rows

    def as_dict(self, target_names=("Negative", "Wakeword")) -> dict:
        """The keys and values of sklearn's classification_report(..., labels=[0, 1], output_dict=True)."""
        p, r, f, s, rows = self._averages()
        out = {name: dict(zip(_HEADERS, (float(p[i]), float(r[i]), float(f[i]), float(s[i])))) for i, name in enumerate(target_names)}
        out["accuracy"] = self.accuracy
        for k, v in rows.items():
            out[k] = dict(zip(_HEADERS, v + [float(s.sum())]))
        return out

    def classification_report(self, target_names=("Negative", "Wakeword"), digits: int = 2) -> str:
        """sklearn's classification_report text for these counts, character for character."""
        if len(target_names) != 2:
            raise ValueError("target_names: two classes")
        p, r, f, s, rows = self._averages()
        width = max(max(len(n) for n in target_names), len("weighted avg"), digits)
        text = "{:>{width}s} ".format("", width=width) + "".join(" {:>9}".format(h) for h in _HEADERS) + "\n\n"
        row_fmt = "{:>{width}s} " + " {:>9.{digits}f}" * 3 + " {:>9}\n"
        for i, name in enumerate(target_names):
            text += row_fmt.format(name, p[i], r[i], f[i], int(s[i]), width=width, digits=digits)
        text += "\n"
        n = int(s.sum())
        text += ("{:>{width}s} " + " {:>9.{digits}}" * 2 + " {:>9.{digits}f}" + " {:>9}\n").format(
            "accuracy", "", "", self.accuracy, n, width=width, digits=digits)
        for k in ("macro avg", "weighted avg"):
            text += row_fmt.format(k, *rows[k], n, width=width, digits=digits)
        return text

    def summary(self) -> dict:
        """The four numbers cell 17 prints: accuracy and the support-weighted precision, recall and F1."""
        w = self._averages()[4]["weighted avg"]
        return {"accuracy": self.accuracy, "precision": w[0], "recall": w[1], "f1": w[2]}

    @property
    def f1(self) -> float:
        """F1 of the wake-word class at argmax."""
        return float(_prf(self.confusion)[2][1])

    # ---- the configured operating points ----
    def at(self, p) -> dict:
        """The counts and rates at one of the configured thresholds (KeyError for any other)."""
        k = None
        if self.thresholds is not None:
            hits = [i for i, q in enumerate(self.thresholds) if q == float(p) or np.float32(q) == np.float32(p)]
            k = hits[0] if hits else None
        if k is None:
            raise KeyError(f"threshold {p!r} is not one of the configured operating points {self.thresholds}")
        (tn, fp), (fn, tp) = (int(x) for x in self.at_counts[k, 0]), (int(x) for x in self.at_counts[k, 1])
        return {"threshold": self.thresholds[k], "margin": float(self.margins[k]), "tp": tp, "fp": fp, "tn": tn, "fn": fn,
                "precision": float(_div(tp, tp + fp)), "recall": float(_div(tp, tp + fn)), "f1": float(_div(2 * tp, 2 * tp + fp + fn)),
                "fpr": float(_div(fp, fp + tn)), "fnr": float(_div(fn, fn + tp))}

    # ---- the curve ----
    def _need_hist(self):
        if self.hist is None:
            raise ValueError("this report was built without a histogram: no ROC, AUC, EER or threshold_for")
        return self.hist

    def roc(self):
        """(fpr, tpr, margins, probabilities) at the 4097 bin edges, from the lowest margin (everything fires) to the highest (nothing does)."""
        h = self._need_hist()
        fired = np.concatenate([np.cumsum(h[:, ::-1], axis=1)[:, ::-1], np.zeros((2, 1), np.int64)], axis=1)   # clips in bins >= j
        neg, pos = int(h[0].sum()), int(h[1].sum())
        edges = bin_edges()
        return _div(fired[0], neg), _div(fired[1], pos), edges, probability_of_margin(edges)

    @property
    def auc(self) -> float:
        """The trapezoid under the 4097 ROC points: the Mann-Whitney statistic of the bin indices, ties counted one half.  NaN without
        both classes."""
        h = self._need_hist()
        if h[0].sum() == 0 or h[1].sum() == 0:
            return float("nan")
        fpr, tpr, _, _ = self.roc()
        return float(np.sum((fpr[:-1] - fpr[1:]) * (tpr[:-1] + tpr[1:])) * 0.5)

    @property
    def auc_bound(self) -> float:
        """sum_b pos_b neg_b / (2 P N): the most that binning can have moved `auc` away from the AUC of the unbinned margins (only pairs
        that share a bin can change, each by at most one half)."""
        h = self._need_hist()
        neg, pos = int(h[0].sum()), int(h[1].sum())
        if neg == 0 or pos == 0:
            return float("nan")
        return float(np.sum(h[0].astype(np.float64) * h[1].astype(np.float64)) / (2.0 * pos * neg))

    @property
    def eer(self) -> float:
        """The equal error rate: walking the ROC points from the lowest edge, g = fpr - fnr falls from 1 to -1; between the last point
        with g >= 0 and the next one, fpr and fnr are interpolated linearly and the EER is their common value where they cross."""
        h = self._need_hist()
        if h[0].sum() == 0 or h[1].sum() == 0:
            return float("nan")
        fpr, tpr, _, _ = self.roc()
        fnr = 1.0 - tpr
        g = fpr - fnr
        j = int(np.nonzero(g >= 0)[0][-1])                 # g[0] = 1 >= 0 and g[-1] = -1 < 0: 0 <= j < 4096
        t = g[j] / (g[j] - g[j + 1])
        return float(fpr[j] + t * (fpr[j + 1] - fpr[j]))

    def threshold_for(self, max_fpr: float):
        """The lowest bin-edge probability whose false-positive rate is at most `max_fpr`, or None (no negative clips).  The edge at +32
        fires nothing, so with negatives there is always one."""
        h = self._need_hist()
        if h[0].sum() == 0:
            return None
        fpr, _, _, prob = self.roc()
        ok = np.nonzero(fpr <= float(max_fpr))[0]
        return float(prob[ok[0]]) if ok.size else None

    # ---- merging ----
    def __add__(self, other):
        if not isinstance(other, ClipReport):
            return NotImplemented
        if self.margins.shape != other.margins.shape or not np.array_equal(self.margins, other.margins):
            raise ValueError("cannot add reports with different operating points")
        if (self.hist is None) != (other.hist is None):
            raise ValueError("cannot add a report with a histogram to one without")
        out = ClipReport(self.confusion + other.confusion, None if self.hist is None else self.hist + other.hist, self.margins.copy(),
                         self.at_counts + other.at_counts, self.bad_labels + other.bad_labels, self.nonfinite + other.nonfinite,
                         self.thresholds if self.thresholds is not None else other.thresholds)
        out.batches = None if self.batches is None or other.batches is None else self.batches + other.batches
        return out

    def __eq__(self, other):
        if not isinstance(other, ClipReport):
            return NotImplemented
        return (np.array_equal(self.confusion, other.confusion) and np.array_equal(self.margins, other.margins)
                and np.array_equal(self.at_counts, other.at_counts) and (self.hist is None) == (other.hist is None)
                and (self.hist is None or np.array_equal(self.hist, other.hist))
                and self.bad_labels == other.bad_labels and self.nonfinite == other.nonfinite)

    __hash__ = None

    def __repr__(self):
        (tn, fp), (fn, tp) = self.confusion.tolist()
        return f"ClipReport(tn={tn}, fp={fp}, fn={fn}, tp={tp}, accuracy={self.accuracy:.4f}, operating_points={len(self.margins)})"

    def cell17(self, target_names=("Negative", "Wakeword")) -> str:
        """The text notebook cell 17 prints: the four headline numbers, then the classification report."""
        s = self.summary()
        return (f"   Accuracy: {s['accuracy']:.4f}\n   Precision: {s['precision']:.4f}\n   Recall: {s['recall']:.4f}\n"
                f"   F1-Score: {s['f1']:.4f}\n\n" + self.classification_report(target_names))
