#!/usr/bin/env python3
"""Reverberation in KA: augmentation throughput with reverb off, on half the clips and on every clip, interleaved in one process at
1 s and 0.5 s, and the RIR bank's build rate.

    PYTHONPATH=. python scripts/bench_reverb.py [--batch 4096] [--steps 10] [--rounds 7] [--out profiles/reverb_bench.json]

Plans are the reference's draws (each transform with probability 0.8, the same plans every step).  Every mode goes through
ww_augment_rir_f32 with prebuilt arrays and no background, so "off" runs exactly ww_augment_f32's / ww_augment_n_f32's launches and the
differences are the reverb kernel.  The goal set for the stage is at most 0.5 ms per 4,096-clip batch with every clip reverberating.
The reverb kernel's own time comes from a kernel trace of this script:
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/bench_reverb.py --steps 3 --rounds 1 --no-build-rate"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import reverb_ref  # noqa: E402  (tests/reverb_ref.py: the synthetic RIRs)
import wakeword_jupyterlab_amd as pkg  # noqa: E402
from wakeword_jupyterlab_amd import _native as nat  # noqa: E402
from wakeword_jupyterlab_amd.reverb import ImpulseResponseBank  # noqa: E402

GOAL_MS = 0.5


def _arrays(plans, bank, rng, share):
    B = len(plans)
    arr = (nat.AugmentPlan * B)()
    rir = (nat.AugmentRir * B)()
    pick = random.Random(3)                   # random clips, as the draws pick them (every other clip would load alternate XCDs only)
    for i, (a, p) in enumerate(zip(arr, plans)):
        a.shift, a.crop_start = p["shift"], p["crop"]
        a.pitch_rate = 2.0 ** (-p["n_steps"] / 12.0) if p["n_steps"] is not None else 0.0
        a.stretch_rate = p["rate"] or 0.0
        a.noise_sigma, a.noise_seed = p["sigma"], p["seed"]
        if share >= 1.0 or (share > 0 and pick.random() < share):
            r = rng.randrange(bank.n_rirs)
            rir[i].index, rir[i].dpos, rir[i].taps, rir[i].enabled = r, int(bank.dpos[r]), int(bank.lengths[r]), 1
    return arr, rir


def measure(n, batch, steps, rounds, dev, bank):
    cfg = type("Cfg", (pkg.AudioConfig,), {"DURATION": n / 16000})
    proc = pkg.AudioProcessor(cfg, device=dev)
    x = pkg.synth.make_clips_tiled(0, batch, unique=64, n=n)
    x = x / np.abs(x).max(axis=1, keepdims=True)
    pcm = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    random.seed(0)
    plans = [proc.draw_augment_plan() for _ in range(batch)]
    modes = {name: _arrays(plans, bank, random.Random(2), share) for name, share in (("off", 0.0), ("half", 0.5), ("all", 1.0))}
    out = torch.empty_like(pcm)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(int(nat.check(nat.lib.ww_augment_rir_workspace_bytes(batch, n))), dtype=torch.uint8, device=dev)

    def run(name):
        arr, rir = modes[name]
        nat.check(nat.lib.ww_augment_rir_f32(pcm.data_ptr(), batch, n, n, arr, None, None, 0, rir, bank.spectra.data_ptr(), bank.n_rirs,
                                             out.data_ptr(), n, ws.data_ptr(), stream))

    def timed(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            run(name)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps
    for name in modes:
        run(name)
    t = {name: [] for name in modes}
    for _ in range(rounds):                                   # interleaved: clock and thermal drift hit every mode alike
        for name in modes:
            t[name].append(timed(name))
    med = {name: statistics.median(v) for name, v in t.items()}
    res = {"n_samples": n, "batch": batch, "steps": steps, "rounds": rounds, "goal_ms_extra_all": GOAL_MS}
    for name in modes:
        res[f"ms_per_batch_{name}"] = med[name] * 1e3
        res[f"ms_{name}_all"] = [v * 1e3 for v in t[name]]
    for name in ("half", "all"):
        res[f"ms_extra_{name}"] = (med[name] - med["off"]) * 1e3
        res[f"cost_pct_{name}"] = 100.0 * (med[name] / med["off"] - 1.0)
    res["meets_goal"] = res["ms_extra_all"] <= GOAL_MS
    return res


def build_rate(dev, files=200):
    """`files` RIR files (half 16 kHz mono PCM-16 of 0.5 s, half 48 kHz mono PCM-16 of 1 s) -> a bank."""
    with tempfile.TemporaryDirectory() as d:
        for i in range(files):
            rate, secs = (16000, 0.5) if i % 2 == 0 else (48000, 1.0)
            h = reverb_ref.decaying_rir(int(rate * secs), 50 + i, seed=i, rt_samples=rate / 6)
            pkg.synth.write_wav16(os.path.join(d, f"rir_{i:04d}.wav"), h * 0.9, sr=rate)
        ImpulseResponseBank(d, device=dev)                                   # warm-up (page cache, kernels)
        bank = ImpulseResponseBank(d, device=dev)
        return dict(bank.stats, bank_bytes=bank.nbytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-build-rate", action="store_true")
    ap.add_argument("--out", default=None, help="also write the result JSON here")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    hs = [reverb_ref.decaying_rir(L, 40 + 7 * i, seed=i, rt_samples=L / 4) for i, L in enumerate((4000, 8000, 12000, 16000, 20000) * 4)]
    bank = ImpulseResponseBank.from_taps(hs, device=dev)
    res = {"device": nat.device_info(), "reverb": [measure(n, a.batch, a.steps, a.rounds, dev, bank) for n in (16000, 8000)]}
    if not a.no_build_rate:
        res["bank_build"] = build_rate(dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
