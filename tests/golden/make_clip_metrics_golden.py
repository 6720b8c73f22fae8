"""Writes tests/golden/clip_metrics_sklearn.json: what scikit-learn says about a few seeded sets of clips.

    python tests/golden/make_clip_metrics_golden.py

Needs scikit-learn (the file was written with 1.7.2); no test runs this.  Each case holds its float32 margins (as their bit patterns, so
they survive JSON exactly) and labels, and sklearn's classification_report (text and output_dict), confusion_matrix and, where both
classes are present, roc_auc_score of the margins' bin indices.  A clip's prediction is 1 iff its margin is > 0.
"""
import json
import os
import sys
import warnings

import numpy as np
from sklearn.metrics import classification_report, confusion_matrix, roc_auc_score

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import metrics_ref as ref  # noqa: E402

NAMES = ["Negative", "Wakeword"]
# (name, seed, clips, fraction of positive labels, spread of the margins, shift of the margins)
CASES = [
    ("one_clip", 1, 1, 1.0, 2.0, 1.0),
    ("no_positive_label", 2, 7, 0.0, 3.0, 0.0),
    ("no_positive_prediction", 3, 50, 0.3, 1.0, None),
    ("balanced_257", 4, 257, 0.5, 4.0, 0.0),
    ("imbalanced_1000", 5, 1000, 0.09, 6.0, 0.0),
    ("wide_2000", 6, 2000, 0.3, 25.0, 0.0),
    ("coarse_300", 7, 300, 0.4, 2.0, 0.0),
]


def make_case(name, seed, n, frac, spread, shift):
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < frac).astype(np.int64)
    d = (rng.standard_normal(n) * spread + (2.0 * y - 1.0) * 0.6 * spread).astype(np.float32)
    if shift is None:
        d = -np.abs(d) - np.float32(0.25)                    # nothing is predicted positive
    if name.startswith("coarse"):
        d = (np.round(d * 4) / 4).astype(np.float32)         # many ties, and margins that sit exactly on bin edges
    pred = (d > 0).astype(np.int64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        text = classification_report(y, pred, labels=[0, 1], target_names=NAMES)
        as_dict = classification_report(y, pred, labels=[0, 1], target_names=NAMES, output_dict=True)
    both = 0 < y.sum() < n
    return {"name": name, "seed": seed, "n": n, "labels": y.tolist(), "margin_bits": d.view(np.uint32).tolist(),
            "confusion": confusion_matrix(y, pred, labels=[0, 1]).tolist(), "report_text": text, "report_dict": as_dict,
            "auc_bins": float(roc_auc_score(y, ref.bins_of(d))) if both else None}


if __name__ == "__main__":
    import sklearn
    out = {"sklearn": sklearn.__version__, "cases": [make_case(*c) for c in CASES]}
    path = os.path.join(HERE, "clip_metrics_sklearn.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")
