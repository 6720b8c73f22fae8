#!/usr/bin/env python3
"""Per-stage errors of the augmentation kernels against float64 (tests/test_gpu_augment_stages.py) -> profiles/aug_stage_errors.json.

    python scripts/aug_stage_errors.py [--json profiles/aug_stage_errors.json]      (needs the MI355X; summary per stage and clip length)"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "aug_stage_errors.json"))
args = ap.parse_args()
raw = args.json + ".raw"
rc = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", os.path.join(ROOT, "tests", "test_gpu_augment_stages.py")],
                    cwd=ROOT, env=dict(os.environ, WW_AUG_STAGE_JSON=raw)).returncode
figs = json.load(open(raw))
os.remove(raw)
out = {}
for f in figs:                                                    # the worst case of every figure, per stage and clip length
    row = out.setdefault(f"{f['stage']} n={f['n']}", {"cases": 0})
    row["cases"] += 1
    for k, v in f.items():
        if k in ("left_out", "bins_unchecked") and not f["share_asserted"]:       # (the half-silent and zero clips: exempt)
            continue
        if isinstance(v, (int, float)) and not isinstance(v, bool) and k != "n":
            row[k] = max(row.get(k, 0), v)
json.dump({"pytest_exit_code": rc, "worst_per_stage_and_length": out}, open(args.json, "w"), indent=1)
print(json.dumps(out, indent=1))
sys.exit(rc)
