#!/usr/bin/env python3
"""The error table of tests/test_gpu_trainer.py as figures: the loss kernel's and the Adam kernel's error against the float64 restatements
of tests/trainer_ref.py, beside torch's own float32 error on the same device and inputs, in units of 2^-24.  Writes
profiles/trainer_errors.json.

    PYTHONPATH=. python scripts/trainer_errors.py [--out profiles/trainer_errors.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import trainer_ref as ref  # noqa: E402
import wakeword_jupyterlab_amd as pkg  # noqa: E402
from wakeword_jupyterlab_amd import ops  # noqa: E402

U = ref.U
DEV = torch.device("cuda", 0)


def ce_rows():
    rows = []
    for n in (1, 2, 63, 64, 65, 257, 4099):
        z, y = ref.ce_inputs(n, seed=n)
        zt, yt = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
        loss, d = ops.ce_loss(zt, yt)
        zr = zt.clone().requires_grad_()
        lt = F.cross_entropy(zr, yt)
        lt.backward()
        l64, d64, _ = ref.ce(z, y)
        rows.append({"n": n, "loss_rel_ours_u": abs(float(loss) - l64) / abs(l64) / U, "loss_rel_torch_u": abs(float(lt.detach()) - l64) / abs(l64) / U,
                     "dlogits_times_n_ours_u": float(np.abs(d.cpu().numpy().astype(np.float64) - d64).max()) * n / U,
                     "dlogits_times_n_torch_u": float(np.abs(zr.grad.cpu().numpy().astype(np.float64) - d64).max()) * n / U})
    return rows


def adam_rows():
    rows = []
    sizes = [1, 2, 3, 4, 5, 255, 256, 257, 65536, 262145]
    for lr in (1e-4, 1e-3):
        for wd in (0.0, 1e-5):
            inputs = [ref.adam_inputs(n, seed=40 + k) for k, n in enumerate(sizes)]
            ps = [torch.from_numpy(p0).to(DEV) for p0, _ in inputs]
            ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
            tps = [torch.nn.Parameter(torch.from_numpy(p0).to(DEV)) for p0, _ in inputs]
            topt = torch.optim.Adam(tps, lr=lr, weight_decay=wd, foreach=False)
            p64 = np.concatenate([p0 for p0, _ in inputs]).astype(np.float64)
            m64, v64, gmax = np.zeros_like(p64), np.zeros_like(p64), 0.0
            for t in range(3):
                gs = [torch.from_numpy(g[t]).to(DEV) for _, g in inputs]
                ops.adam_step(ps, gs, ms, vs, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, step=t + 1)
                for p, g in zip(tps, gs):
                    p.grad = g.clone()
                topt.step()
                p64, m64, v64, g1 = ref.adam_step(p64, np.concatenate([g[t] for _, g in inputs]), m64, v64, lr, 0.9, 0.999, 1e-8, wd, t + 1)
                gmax = max(gmax, float(np.abs(g1).max()))
            cat = lambda ts: np.concatenate([x.detach().cpu().numpy() for x in ts])        # noqa: E731
            eo = ref.adam_errors(cat(ps), cat(ms), cat(vs), p64, m64, v64, lr, gmax)
            et = ref.adam_errors(cat(tps), cat([topt.state[p]["exp_avg"] for p in tps]), cat([topt.state[p]["exp_avg_sq"] for p in tps]),
                                 p64, m64, v64, lr, gmax)
            rows.append({"lr": lr, "weight_decay": wd, "steps": 3, **{f"{k}_ours_u": e / U for k, e in zip("pmv", eo)},
                         **{f"{k}_torch_u": e / U for k, e in zip("pmv", et)}})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trainer_errors.json"))
    a = ap.parse_args()
    out = {"unit": "2^-24", "rule": "ours <= 2 x torch + 1; torch under its cap (tests/trainer_ref.py)",
           "caps_u": {"p": ref.CAP_P / U, "m": ref.CAP_M / U, "v": ref.CAP_V / U, "dlogits_times_n": ref.CAP_DLOGITS / U, "loss_rel": ref.CAP_LOSS / U},
           "device": pkg._native.device_info(), "torch": torch.__version__, "cross_entropy": ce_rows(), "adam": adam_rows()}
    for key in ("cross_entropy", "adam"):
        for r in out[key]:
            print(json.dumps(r))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
