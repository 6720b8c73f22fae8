"""CPU-only checks of clip evaluation: metrics.ClipReport against the reference notebook's recorded cell 17, against scikit-learn's
recorded answers (tests/golden/clip_metrics_sklearn.json, written by tests/golden/make_clip_metrics_golden.py) and against the numpy
restatement (tests/metrics_ref.py); and the host side of the ww_clip_metrics_* entry points, which need no GPU."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import metrics_ref as ref
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd.metrics import ClipReport

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HAS_GPU = torch.cuda.is_available()
CELL17 = [[1124, 17], [12, 517]]


def _margins(thresholds):
    return np.array([nat.lib.ww_clip_metrics_margin_host(p) for p in thresholds], np.float32)


def _report(d, y, thresholds=(0.5, 0.8, 0.999)):
    """A ClipReport from margins and labels through the restatement's counters (logits (0, d))."""
    z = np.stack([np.zeros_like(d), d], axis=1).astype(np.float32)
    m = _margins(thresholds)
    c = ref.counters(z, y, m)
    return ClipReport.from_counts(c["argmax"], hist=c["hist"], margins=m, at=c["at"], bad_labels=c["bad_labels"], nonfinite=c["nonfinite"],
                                  thresholds=thresholds), c


def test_cell17_recorded_output_comes_from_exactly_one_confusion_matrix():
    want = open(os.path.join(GOLDEN, "cell17_report.txt")).read()
    head, _, text = want.partition("\n\n")
    heads = [line.split(": ")[1] for line in head.splitlines()]
    assert heads == ["0.9826", "0.9827", "0.9826", "0.9827"]
    r = ClipReport.from_counts(CELL17)
    assert r.classification_report() == text and r.cell17() == want
    s = r.summary()
    assert [f"{s[k]:.4f}" for k in ("accuracy", "precision", "recall", "f1")] == heads
    assert r.total == 1670 and r.support.tolist() == [1141, 529] and r.accuracy == (1124 + 517) / 1670
    hits = []
    for fn in range(81):
        for fp in range(81 - fn):
            q = ClipReport.from_counts([[1141 - fp, fp], [fn, 529 - fn]])
            qs = q.summary()
            if [f"{qs[k]:.4f}" for k in ("accuracy", "precision", "recall", "f1")] == heads and q.classification_report() == text:
                hits.append((fn, fp))
    assert hits == [(12, 17)]


def _cases():
    return json.load(open(os.path.join(GOLDEN, "clip_metrics_sklearn.json")))["cases"]


def _close(a, b):
    if isinstance(b, dict):
        assert sorted(a) == sorted(b)
        for k in b:
            _close(a[k], b[k])
    else:
        assert abs(a - b) <= 1e-12, (a, b)


@pytest.mark.parametrize("index", range(7))
def test_sklearn_cases(index):
    case = _cases()[index]
    d = np.array(case["margin_bits"], np.uint32).view(np.float32)
    y = np.array(case["labels"], np.int64)
    assert len(d) == len(y) == case["n"]
    r, c = _report(d, y)
    assert r.confusion.tolist() == case["confusion"]
    assert r.classification_report() == case["report_text"] == ref.report_text(r.confusion)
    _close(r.as_dict(), case["report_dict"])
    _close(r.as_dict(), ref.report_dict(r.confusion))
    if case["auc_bins"] is None:
        assert math.isnan(r.auc) and math.isnan(r.eer) and math.isnan(r.auc_bound)
    else:
        assert abs(r.auc - case["auc_bins"]) <= 1e-12 and abs(r.auc - ref.auc_binned(c["hist"])) <= 1e-12
        assert abs(r.eer - ref.eer(c["hist"])) <= 1e-12
    fpr, tpr, edges, prob = r.roc()
    rf, rt = ref.roc(c["hist"])
    assert fpr.shape == tpr.shape == edges.shape == prob.shape == (4097,)
    assert np.abs(fpr - rf).max() <= 1e-12 and np.abs(tpr - rt).max() <= 1e-12
    assert edges[0] == -32.0 and edges[-1] == 32.0 and edges[2048] == 0.0 and prob[2048] == 0.5 and np.all(np.diff(prob) > 0)
    # the operating points: a clip fires iff its float32 margin is >= the library's float32 margin
    for p, m in zip((0.5, 0.8, 0.999), _margins((0.5, 0.8, 0.999))):
        a = r.at(p)
        fired = d >= m
        assert (a["tp"], a["fp"], a["tn"], a["fn"]) == (int((fired & (y == 1)).sum()), int((fired & (y == 0)).sum()),
                                                        int((~fired & (y == 0)).sum()), int((~fired & (y == 1)).sum()))
        assert a["fpr"] == (a["fp"] / (a["fp"] + a["tn"]) if (y == 0).any() else 0.0)
        assert a["recall"] == (a["tp"] / (a["tp"] + a["fn"]) if (y == 1).any() else 0.0) and a["margin"] == float(m)
    with pytest.raises(KeyError):
        r.at(0.7)


def test_the_sklearn_file_has_the_degenerate_cases():
    cases = _cases()
    assert 6 <= len(cases) <= 8 and len(cases) == 7
    assert min(c["n"] for c in cases) == 1 and max(c["n"] for c in cases) == 2000
    assert any(sum(c["labels"]) == 0 for c in cases) and any(c["confusion"][0][1] + c["confusion"][1][1] == 0 for c in cases)


@pytest.mark.parametrize("seed,n,spread", [(11, 500, 1.0), (12, 3000, 5.0), (13, 2000, 0.05), (14, 400, 30.0)])
def test_binned_auc_is_within_its_bound_of_the_exact_auc(seed, n, spread):
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < 0.2).astype(np.int64)
    d = (rng.standard_normal(n) * spread + (2.0 * y - 1.0) * spread * 0.5).astype(np.float32)
    r, c = _report(d, y)
    exact = ref.auc_exact(d, y)
    print(f"auc {r.auc:.9f} exact {exact:.9f} bound {r.auc_bound:.3e}")
    assert r.auc_bound == ref.auc_bound(c["hist"])
    h = c["hist"].astype(np.float64)
    assert r.auc_bound == float(np.sum(h[0] * h[1]) / (2.0 * h[0].sum() * h[1].sum()))
    assert abs(r.auc - exact) <= r.auc_bound + 1e-15           # 1e-15: the two sums round differently in float64


def test_threshold_for_and_eer_on_a_hand_made_histogram():
    hist = np.zeros((2, 4096), np.int64)
    hist[0, [100, 2000, 2100, 3000]] = [6, 2, 1, 1]            # 10 negatives
    hist[1, [1900, 2100, 3500]] = [1, 1, 2]                    # 4 positives
    r = ClipReport.from_counts([[8, 2], [1, 3]], hist=hist)
    fpr, tpr, edges, prob = r.roc()
    assert fpr[0] == 1.0 and tpr[0] == 1.0 and fpr[-1] == 0.0 and tpr[-1] == 0.0
    assert fpr[101] == 0.4 and fpr[2001] == 0.2 and fpr[2101] == 0.1 and fpr[3001] == 0.0 and tpr[1901] == 0.75 and tpr[2101] == 0.5
    assert r.threshold_for(0.1) == prob[2101] and r.threshold_for(0.0) == prob[3001] and r.threshold_for(1.0) == prob[0]
    assert r.threshold_for(0.39) == prob[2001]
    assert ClipReport.from_counts([[0, 0], [1, 3]], hist=hist * np.array([[0], [1]])).threshold_for(0.5) is None
    # pairs: positives at 1900 beat 6, at 2100 beat 8 and tie 1, at 3500 beat 10 each
    assert abs(r.auc - (6 + 8.5 + 20) / 40) <= 1e-15 and abs(r.auc - ref.auc_binned(hist)) <= 1e-15
    assert r.auc_bound == 1 / 80
    # fpr - fnr: edge 1901 gives 0.4 - 0.25 > 0 ... edge 2001 gives 0.2 - 0.25 < 0; crossing between edges 2000 and 2001
    assert abs(r.eer - ref.eer(hist)) <= 1e-15 and abs(r.eer - (0.4 + (0.15 / 0.2) * (0.2 - 0.4))) <= 1e-15
    with pytest.raises(ValueError):
        ClipReport.from_counts(CELL17).roc()


def test_merge_adds_every_counter():
    rng = np.random.default_rng(5)
    y = rng.integers(0, 2, 700)
    y[::50] = 7                                                # bad labels
    d = (rng.standard_normal(700) * 8).astype(np.float32)
    d[3], d[9] = np.inf, np.nan
    a, _ = _report(d[:300], y[:300])
    b, _ = _report(d[300:], y[300:])
    whole, c = _report(d, y)
    s = a + b
    assert s == whole and whole.bad_labels == 14 and whole.nonfinite == 2 and s.clips_seen == 700
    ref.assert_counters(s, c)
    assert s.auc == whole.auc and s.at(0.8) == whole.at(0.8)
    other, _ = _report(d, y, thresholds=(0.5, 0.9, 0.999))
    with pytest.raises(ValueError):
        a + other
    with pytest.raises(ValueError):
        a + ClipReport.from_counts(CELL17)
    assert a != b


def test_from_counts_refuses_what_is_not_a_count():
    for bad in ([[1, 2], [3]], [[1.5, 0], [0, 1]], [[1, -1], [0, 1]], [[1, 2, 3], [4, 5, 6]]):
        with pytest.raises(ValueError):
            ClipReport.from_counts(bad)
    with pytest.raises(ValueError):
        ClipReport.from_counts(CELL17, hist=np.zeros((2, 100), np.int64))
    with pytest.raises(ValueError):
        ClipReport.from_counts(CELL17, margins=(0.0,), at=None)
    empty = ClipReport.from_counts([[0, 0], [0, 0]])
    assert empty.accuracy == 0.0 and empty.summary() == {"accuracy": 0.0, "precision": 0.0, "recall": 0.0, "f1": 0.0}


def test_argument_checks_return_einval_before_any_hip_call():
    assert nat.lib.ww_clip_metrics_bytes() == C.sizeof(nat.ClipMetrics) == 8 * (8 + 32 + 2 * 4096) + 4 * 8 + 8
    assert nat.METRICS_BINS == 4096 and nat.METRICS_MAX_THRESHOLDS == 8
    buf = np.zeros(nat.lib.ww_clip_metrics_bytes() // 8 + 2, np.int64)
    base = buf.ctypes.data
    upd, init, reset = nat.lib.ww_clip_metrics_update_f32, nat.lib.ww_clip_metrics_init, nat.lib.ww_clip_metrics_reset

    def einval(rc, word):
        assert rc == nat.WW_EINVAL and word in nat.lib.ww_last_error(), (rc, nat.lib.ww_last_error())
    einval(upd(base, base, -1, base, None), b"n -1")
    einval(upd(base, base, (1 << 30) + 1, base, None), b"n ")
    einval(upd(None, base, 4, base, None), b"null logits_dev")
    einval(upd(base, None, 4, base, None), b"null logits_dev / labels_dev")
    einval(upd(base + 4, base, 4, base, None), b"logits_dev must be 8-byte")
    einval(upd(base, base + 4, 4, base, None), b"labels_dev must be 8-byte")
    einval(upd(base, base, 4, None, None), b"null state_dev")
    einval(upd(base, base, 4, base + 4, None), b"state_dev must be 8-byte")
    einval(upd(base, base, 0, base + 4, None), b"state_dev must be 8-byte")       # the checks come before the n == 0 return
    assert upd(base, base, 0, base, None) == nat.WW_OK                            # nothing to launch: no device needed
    thr = (C.c_float * 9)(*([0.5] * 9))
    einval(init(None, thr, 1, None), b"null state_dev")
    einval(init(base + 2, thr, 1, None), b"state_dev must be 8-byte")
    einval(init(base, thr, 9, None), b"n_thresholds 9")
    einval(init(base, thr, -1, None), b"n_thresholds -1")
    einval(init(base, None, 1, None), b"null thresholds_host")
    for bad in (0.0, 1.0, -0.25, 1.5, float("nan"), float("inf")):
        thr[2] = bad
        einval(init(base, thr, 3, None), b"thresholds_host[2]")
        assert math.isnan(nat.lib.ww_clip_metrics_margin_host(bad)) and b"p " in nat.lib.ww_last_error()
    einval(reset(None, None), b"null state_dev")
    einval(reset(base + 1, None), b"state_dev must be 8-byte")
    if not HAS_GPU:                                            # valid arguments: only the device is missing
        thr[2] = 0.5
        assert init(base, thr, 3, None) == nat.WW_ENODEVICE and init(base, None, 0, None) == nat.WW_ENODEVICE
        assert reset(base, None) == nat.WW_ENODEVICE and upd(base, base, 4, base, None) == nat.WW_ENODEVICE
        assert not buf.any()                                   # and nothing was written


def test_margin_of_a_threshold():
    f = nat.lib.ww_clip_metrics_margin_host
    assert f(0.5) == 0.0
    ps = np.unique(np.concatenate([np.linspace(1e-6, 1 - 1e-6, 4001), [0.8, 0.999, 0.9999999, 1e-30, np.nextafter(np.float32(1), np.float32(0))]])
                   .astype(np.float32))
    ms = np.array([f(float(p)) for p in ps], np.float64)
    assert np.all(np.isfinite(ms)) and np.all(np.diff(ms) >= 0) and np.all(np.diff(ms[::40]) > 0)
    # (float)log(p / (1 - p)) with p the float32 value, evaluated in double
    want = np.array([np.float32(math.log(float(p) / (1.0 - float(p)))) for p in ps], np.float64)
    assert np.array_equal(ms, want)
    assert f(0.8) == np.float32(math.log(float(np.float32(0.8)) / (1.0 - float(np.float32(0.8)))))
    assert f(0.75) == -f(0.25)
