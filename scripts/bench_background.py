#!/usr/bin/env python3
"""Background noise in KA: augmentation throughput with the mix off and on (every clip mixing), interleaved in one process at 1 s and
0.5 s, and the noise bank's build rate.

    PYTHONPATH=. python scripts/bench_background.py [--batch 4096] [--steps 10] [--rounds 7] [--out profiles/background_bench.json]

Plans are the reference's draws (each transform with probability 0.8, the same plans every step); "on" adds a background segment to
every clip.  Both modes go through the C ABI with prebuilt plan arrays (ww_augment_f32 / ww_augment_n_f32 vs ww_augment_bg_f32), so the
difference is the mix kernel replacing the Gaussian-noise kernel.  The mix kernel's own time comes from a kernel trace of this script:
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/bench_background.py --steps 3 --rounds 1 --no-build-rate"""
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
import numpy as np  # noqa: E402
import torch  # noqa: E402

import wakeword_jupyterlab_amd as pkg  # noqa: E402
from wakeword_jupyterlab_amd import _native as nat  # noqa: E402
from wakeword_jupyterlab_amd.background import BackgroundNoiseBank  # noqa: E402


def _arrays(plans, bank, rng):
    B = len(plans)
    arr = (nat.AugmentPlan * B)()
    bg = (nat.AugmentBg * B)()
    for a, b, p in zip(arr, bg, plans):
        a.shift, a.crop_start = p["shift"], p["crop"]
        a.pitch_rate = 2.0 ** (-p["n_steps"] / 12.0) if p["n_steps"] is not None else 0.0
        a.stretch_rate = p["rate"] or 0.0
        a.noise_sigma, a.noise_seed = p["sigma"], p["seed"]
        f = rng.randrange(bank.n_files)
        b.file_offset, b.file_len = int(bank.offsets[f]), int(bank.lengths[f])
        b.start, b.snr_db, b.enabled = rng.randrange(int(bank.lengths[f])), rng.uniform(0.0, 40.0), 1
    return arr, bg


def measure_mix(n, batch, steps, rounds, dev):
    cfg = type("Cfg", (pkg.AudioConfig,), {"DURATION": n / 16000})
    proc = pkg.AudioProcessor(cfg, device=dev)
    x = pkg.synth.make_clips_tiled(0, batch, unique=64, n=n)
    x = x / np.abs(x).max(axis=1, keepdims=True)
    pcm = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    random.seed(0)
    plans = [proc.draw_augment_plan() for _ in range(batch)]
    rng = np.random.default_rng(1)
    noise = [(rng.standard_normal(5 * 16000) * 0.1).astype(np.float32) for _ in range(20)]    # create_sample_data's 20 x 5 s
    bank = BackgroundNoiseBank.from_buffer(torch.from_numpy(np.concatenate(noise)).to(dev), [len(f) for f in noise])
    arr, bg = _arrays(plans, bank, random.Random(2))
    out = torch.empty_like(pcm)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(int(nat.check(nat.lib.ww_augment_bg_workspace_bytes(batch, n))), dtype=torch.uint8, device=dev)

    def off():
        if n == 16000:
            nat.check(nat.lib.ww_augment_f32(pcm.data_ptr(), batch, n, arr, out.data_ptr(), ws.data_ptr(), stream))
        else:
            nat.check(nat.lib.ww_augment_n_f32(pcm.data_ptr(), batch, n, n, arr, out.data_ptr(), n, ws.data_ptr(), stream))

    def on():
        nat.check(nat.lib.ww_augment_bg_f32(pcm.data_ptr(), batch, n, n, arr, bg, bank.data.data_ptr(), bank.data.numel(), out.data_ptr(), n,
                                            ws.data_ptr(), stream))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps
    off(), on()
    t_off, t_on = [], []
    for _ in range(rounds):                                   # interleaved: clock and thermal drift hit both modes alike
        t_off.append(timed(off))
        t_on.append(timed(on))
    m_off, m_on = statistics.median(t_off), statistics.median(t_on)
    return {"n_samples": n, "batch": batch, "steps": steps, "rounds": rounds,
            "ms_per_batch_off": m_off * 1e3, "ms_per_batch_on": m_on * 1e3,
            "clips_per_s_off": batch / m_off, "clips_per_s_on": batch / m_on, "cost_pct": 100.0 * (m_on / m_off - 1.0),
            "ms_off_all": [t * 1e3 for t in t_off], "ms_on_all": [t * 1e3 for t in t_on]}


def build_rate(dev, files=200, seconds=5.0):
    """`files` noise files of `seconds` each (half 16 kHz mono PCM-16 as create_sample_data writes, half 44.1 kHz stereo) -> a bank."""
    import struct
    rng = np.random.default_rng(3)
    with tempfile.TemporaryDirectory() as d:
        for i in range(files):
            rate, ch = (16000, 1) if i % 2 == 0 else (44100, 2)
            x = np.clip(rng.standard_normal((int(rate * seconds), ch)) * 3000, -32768, 32767).astype("<i2")
            raw = x.tobytes()
            hdr = (b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " +
                   struct.pack("<IHHIIHH", 16, 1, ch, rate, rate * ch * 2, ch * 2, 16) + b"data" + struct.pack("<I", len(raw)))
            with open(os.path.join(d, f"noise_{i:04d}.wav"), "wb") as f:
                f.write(hdr + raw)
        BackgroundNoiseBank(d, device=dev, max_seconds=1.0)                   # warm-up (page cache, kernels)
        bank = BackgroundNoiseBank(d, device=dev)
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
    res = {"device": nat.device_info(), "mix": [measure_mix(n, a.batch, a.steps, a.rounds, dev) for n in (16000, 8000)]}
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
