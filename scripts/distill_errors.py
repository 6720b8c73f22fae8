#!/usr/bin/env python3
"""The error table of the distillation tests (tests/test_gpu_distill.py) as figures: over every case of distill_ref.grid() at the sizes of
distill_ref.SIZES, the largest error of ww_distill_loss_f32 against the float64 restatement of tests/distill_ref.py, as a multiple of the
bound the tests assert (|loss - ref| <= 2^-23 |ref| + 1e-12; per gradient element 2^-23 |ref| + 1e-12 x the terms' factors over their
denominators), and beside it the same formula composed from torch's float32 pieces on the device (F.cross_entropy / FocalLoss +
F.kl_div(..., "batchmean") * T^2 with autograd): what a hand-written loss costs in accuracy.  A figure at or below 1 is inside the bound.
Needs a GPU.  Writes profiles/distill_errors.json.

    PYTHONPATH=. python scripts/distill_errors.py [--out profiles/distill_errors.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import distill_ref as ref  # noqa: E402


def ratios(loss, d, want):
    """(loss error, largest gradient-element error), each over its bound; a NaN on one side only is infinite."""
    if loss != loss or want["loss"] != want["loss"]:
        e_loss = 0.0 if (loss != loss and want["loss"] != want["loss"]) else float("inf")
    else:
        e_loss = abs(loss - want["loss"]) / ref.loss_bound(want["loss"])
    e_d = float((np.abs(np.asarray(d, np.float64) - want["dlogits"]) / np.maximum(ref.dlogits_bound(want), 1e-300)).max())
    return e_loss, e_d


def run(device):
    from wakeword_jupyterlab_amd import ops
    from wakeword_jupyterlab_amd.loss import FocalLoss
    worst = {"kernel": {"loss": 0.0, "dlogits": 0.0}, "torch_float32": {"loss": 0.0, "dlogits": 0.0}}
    where = {"kernel": {}, "torch_float32": {}}
    cases = 0
    for n in ref.SIZES:
        z, zt, y, t = ref.inputs(n)
        zd, ztd, yd, td = (torch.from_numpy(a).to(device) for a in (z, zt, y, t))
        for tag, kind, opts, alpha, T in ref.grid():
            target = ref.target_of(kind, y, t)
            want = ref.distill(z, zt, target, alpha, T, **opts)
            lo, do = ops.distill_loss(zd, ztd, ref.target_of(kind, yd, td), alpha=alpha, temperature=T, **opts)
            lt, dt = ref.torch_formula(z, zt, target, alpha, T, opts, device, torch.float32, FocalLoss)
            if want["loss"] != want["loss"]:
                lt = float("nan")                        # the composition has no rule for a batch in which nothing counts
            for who, (loss, d) in (("kernel", (float(lo), do.cpu().numpy())), ("torch_float32", (lt, dt))):
                for q, v in zip(("loss", "dlogits"), ratios(loss, d, want)):
                    if v > worst[who][q]:
                        worst[who][q], where[who][q] = v, f"{tag} n={n}"
            cases += 1
    return {"cases": cases, "worst_error_over_bound": worst, "where": where}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_errors.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distill_errors.py measures on the MI355X: no GPU is visible")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    from wakeword_jupyterlab_amd import _native as nat
    out = {"bounds": "loss: 2^-23 |ref| + 1e-12; dlogits element: 2^-23 |ref| + 1e-12 (alpha T / D_kd + (1 - alpha) max(w, 1) / D_hard)",
           "unit": "error / bound (<= 1 passes tests/test_gpu_distill.py)", "sizes": list(ref.SIZES), "temperatures": list(ref.TEMPERATURES),
           "alphas": list(ref.ALPHAS), "option_sets": [tag for tag, _, _ in ref.OPTION_SETS], "torch": torch.__version__,
           "device": nat.device_info()}
    out.update(run(device))
    print(json.dumps(out["worst_error_over_bound"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
