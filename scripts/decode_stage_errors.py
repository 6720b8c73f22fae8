#!/usr/bin/env python3
"""Per-rate errors of K0's resampler against float64 on its own input (tests/test_gpu_decode_stages.py) -> profiles/k0_stage_errors.json.

    python scripts/decode_stage_errors.py [--json profiles/k0_stage_errors.json]      (needs the MI355X)

Per rate: max |got - y| / (n u A) (the share of the derived bound the kernel uses; above 1 is a finding), the largest product count, and
max |got - scipy.signal.resample_poly|."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "k0_stage_errors.json"))
args = ap.parse_args()
raw = args.json + ".raw"
rc = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", os.path.join(ROOT, "tests", "test_gpu_decode_stages.py")],
                    cwd=ROOT, env=dict(os.environ, WW_K0_STAGE_JSON=raw)).returncode
figs = json.load(open(raw))
os.remove(raw)
out = {"pytest_exit_code": rc, "largest_ratio_of_n_u_A": max(f["max_ratio_of_n_u_A"] for f in figs), "per_rate": {str(f.pop("rate")): f for f in figs}}
json.dump(out, open(args.json, "w"), indent=1)
print(json.dumps(out, indent=1))
sys.exit(rc)
