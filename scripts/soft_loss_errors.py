#!/usr/bin/env python3
"""The error table of the soft-target loss tests (tests/test_gpu_mixup.py) as figures, and where their caps come from: torch's float32
error of F.cross_entropy with probability targets against the float64 restatement of tests/mixup_ref.py over every case (weights x
smoothing x reductions at the sizes of loss_ref.SIZES), in units of 2^-24 -- with torch on the CPU (no GPU needed: these figures set
the caps, the next power of two at or above twice the largest, per quantity), and on a GPU the same for torch on the device beside the
error of ww_ce_loss_soft_f32.  Each run replaces its own section of profiles/soft_loss_errors.json and keeps the other.

    PYTHONPATH=. python scripts/soft_loss_errors.py [--device cpu|cuda] [--out profiles/soft_loss_errors.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import loss_ref  # noqa: E402
import mixup_ref as ref  # noqa: E402

U = ref.U
QUANTITIES = ("soft_loss_rel", "soft_dlogits")


def next_pow2_at_or_above(x):
    return float(2.0 ** np.ceil(np.log2(x))) if x > 0 else 0.0


def run(device):
    on_gpu = device.type == "cuda"
    if on_gpu:
        from wakeword_jupyterlab_amd import ops
    worst = {f"{q}_torch_u": 0.0 for q in QUANTITIES}
    if on_gpu:
        worst.update({f"{q}_ours_u": 0.0 for q in QUANTITIES})
    rows = []
    for n in loss_ref.SIZES:
        z, t = ref.soft_inputs(n)
        for case in ref.soft_cases(n):
            want = ref.restate(case, z, t)
            lt, dt = ref.torch_reference(case, z, t, device)
            row = {"case": case["tag"], "soft_loss_rel_torch_u": loss_ref.loss_error(lt, want["loss"]) / U,
                   "soft_dlogits_torch_u": loss_ref.dlogits_error(dt, want) / U}
            if on_gpu:
                lo, do = ops.soft_ce_loss(torch.from_numpy(z).to(device), torch.from_numpy(t).to(device), **case["opts"])
                row["soft_loss_rel_ours_u"] = loss_ref.loss_error(float(lo), want["loss"]) / U
                row["soft_dlogits_ours_u"] = loss_ref.dlogits_error(do.cpu().numpy(), want) / U
            for k, v in row.items():
                if k != "case":
                    worst[k] = max(worst[k], v)
            rows.append(row)
    section = {"torch": torch.__version__, "cases": len(rows), "worst": worst}
    if on_gpu:
        from wakeword_jupyterlab_amd import _native as nat
        section["device"] = nat.device_info()
    else:
        section["caps_by_the_recipe_u"] = {q: next_pow2_at_or_above(2.0 * worst[f"{q}_torch_u"]) for q in QUANTITIES}
    section["rows_above_1u"] = [r for r in rows if any(v > 1.0 for k, v in r.items() if k != "case")]
    return section


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_loss_errors.json"))
    a = ap.parse_args()
    device = torch.device(a.device)
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out["unit"] = "2^-24"
    out["rule"] = "ours <= 2 x torch + 1; torch under its cap (tests/mixup_ref.py); caps: next power of two >= 2 x the CPU run's worst figure"
    out["caps_u"] = {"soft_loss_rel": ref.CAP_SOFT_LOSS / U, "soft_dlogits": ref.CAP_SOFT_DLOGITS / U}
    key = "torch_on_gpu_and_kernel" if device.type == "cuda" else "torch_on_cpu"
    out[key] = run(device)
    print(json.dumps({key: out[key]["worst"]}))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
