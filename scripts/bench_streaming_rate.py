#!/usr/bin/env python3
"""Streaming at the microphone's own rate: the per-hop cost of converting and resampling the hop in the graph's first node, against
the 16 kHz float32 mono detector, 256 microphones, 10 ms hops, 1 s windows, all in one process.  The configurations run in
interleaved rounds (every round measures each once, in rotating order) so that clock drift and warm-up fall on all alike; per
configuration the median over rounds of each round's p50 / p99 latency (host enqueue -> results ready), back-to-back hops/s and
device time per replay.

    PYTHONPATH=. python scripts/bench_streaming_rate.py [--mics 256] [--hops 1000] [--rounds 5]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import wakeword_jupyterlab_amd as pkg  # noqa: E402

# (label, sample rate, channels, dtype, input frames per hop): 10 ms hops, 160 samples at 16 kHz (8,820 Hz: 50 ms, 800 samples)
CONFIGS = [("16k_f32_mono", 16000, 1, torch.float32, 160), ("48k_s16_mono", 48000, 1, torch.int16, 480),
           ("44.1k_s16_stereo", 44100, 2, torch.int16, 441), ("11.025k_s16_mono", 11025, 1, torch.int16, 441),
           ("8.82k_s16_mono", 8820, 1, torch.int16, 441)]   # the one with its taps in global memory (16,001 taps: not in LDS)


def _model(dev):
    m = pkg.SimpleWakewordModel()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in pkg.synth.make_state_dict("simple", seed=1234).items()})
    return m.to(dev).eval()


def _setup(m, dev, mics, rate, channels, dtype, hop):
    det = pkg.StreamingDetector(m, n_mics=mics, hop_samples=hop, sample_rate=rate, channels=channels, dtype=dtype)
    g = torch.Generator().manual_seed(rate + channels)
    x = 0.3 * torch.randn((mics, 64 * hop, channels), generator=g)
    x = (x * 32767).round().clamp(-32768, 32767).to(torch.int16) if dtype == torch.int16 else x
    if channels == 1:
        x = x[..., 0]
    hops = [x[:, k * hop:(k + 1) * hop].contiguous().to(dev) for k in range(64)]
    for k in range(100):                                    # one second of 10 ms hops: a whole window
        det.step(hops[k % 64])
    det.stream.synchronize()
    return det, hops


def _once(det, hops, n):
    lat = np.empty(n)
    for k in range(n):
        t0 = time.perf_counter()
        det.step(hops[k % 64])
        det.stream.synchronize()
        lat[k] = time.perf_counter() - t0
    t0 = time.perf_counter()
    for k in range(n):
        det.step(hops[k % 64])
    det.stream.synchronize()
    thr = n / (time.perf_counter() - t0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with torch.cuda.stream(det.stream):
        ev[0].record()
        for k in range(100):
            det.step()
        ev[1].record()
    det.stream.synchronize()
    return {"p50_us": float(np.percentile(lat, 50) * 1e6), "p99_us": float(np.percentile(lat, 99) * 1e6), "hops_per_s": thr,
            "device_us_per_replay": ev[0].elapsed_time(ev[1]) * 10.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mics", type=int, default=256)
    ap.add_argument("--hops", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, help="one configuration by label (e.g. for a kernel trace of it alone)")
    args = ap.parse_args()
    configs = [c for c in CONFIGS if args.only in (None, c[0])]
    if not configs:
        ap.error(f"--only {args.only}: labels are {', '.join(c[0] for c in CONFIGS)}")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    m = _model(dev)
    runs = {c[0]: _setup(m, dev, args.mics, *c[1:]) for c in configs}
    for det, hops in runs.values():                         # warm-up round, not kept
        _once(det, hops, 200)
    per = {c[0]: [] for c in configs}
    for r in range(args.rounds):
        order = configs[r % len(configs):] + configs[:r % len(configs)]
        for c in order:
            per[c[0]].append(_once(*runs[c[0]], args.hops))
    out = {"mics": args.mics, "hops": args.hops, "rounds": args.rounds, "device": torch.cuda.get_device_name(dev), "configs": {}}
    for label, rate, channels, dtype, hop in configs:
        det = runs[label][0]
        med = {k: float(np.median([r[k] for r in per[label]])) for k in per[label][0]}
        med.update(sample_rate=rate, channels=channels, dtype=str(dtype).replace("torch.", ""), hop_frames=hop,
                   latency_samples=det.latency_samples, finite_probs=int(torch.isfinite(det.prob).sum().item()))
        out["configs"][label] = med
    if CONFIGS[0][0] in out["configs"]:
        base = out["configs"][CONFIGS[0][0]]["device_us_per_replay"]
        for label in out["configs"]:
            out["configs"][label]["device_us_over_16k"] = out["configs"][label]["device_us_per_replay"] - base
    for det, _ in runs.values():
        det.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
