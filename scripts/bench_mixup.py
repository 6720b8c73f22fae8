#!/usr/bin/env python3
"""What mixup and class-probability targets cost on the MI355X, three measurements in one process:

  kernel   ww_mixup_f32 at B = 4096, T = 32 with half and with all rows mixed, beside `out.copy_(mel)` of the same batch: device events
           around `--launches` back-to-back calls per window, the three variants alternating window by window after a warm-up window
           each; microseconds per call, the bytes each variant must move (copy 2 x batch; mixup 2 x batch + the partner rows of the mixed
           rows, at most 1.5 x the copy's) and the rate they give
  step     WakewordTrainer.step with float32 [B, 2] targets beside the same step with int64 labels, both models, B = 16 and B = 4096,
           T = 32: two trainers on their own copy of the model, alternating windows that end in a synchronise
  loader   one epoch of bank.loader(augment=True) over `--clips` synthetic 1 s clips with set_mixup on and off, alternating epochs

Every figure is the median over the windows with their spread (min .. max).  Writes profiles/mixup_bench.json.

    PYTHONPATH=. python scripts/bench_mixup.py [--launches 50] [--windows 9] [--clips 1024] [--out profiles/mixup_bench.json]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import wakeword_jupyterlab_amd as pkg  # noqa: E402
from wakeword_jupyterlab_amd import _native as nat  # noqa: E402
from wakeword_jupyterlab_amd import ops  # noqa: E402
from wakeword_jupyterlab_amd.config import MixupConfig  # noqa: E402


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def bench_kernel(dev, launches, windows, B=4096, T=32):
    g = torch.Generator().manual_seed(0)
    mel = (-80.0 * torch.rand(B, 1, 80, T, generator=g)).to(dev)
    out = torch.empty_like(mel)
    targets = torch.empty(B, 2, device=dev)
    labels = torch.randint(0, 2, (B,), generator=g).to(dev)
    rng = np.random.default_rng(0)
    batch_bytes = mel.numel() * 4
    variants = {"copy": (lambda: out.copy_(mel), 2 * batch_bytes, 0)}
    for name, prob in (("mixup_prob_0.5", 0.5), ("mixup_prob_1.0", 1.0)):
        chosen = rng.random(B) < prob
        lam = torch.from_numpy(np.where(chosen, 0.5 + 0.499 * rng.random(B), 1.0).astype(np.float32)).to(dev)
        partner = torch.from_numpy(np.where(chosen, rng.permutation(B), np.arange(B)).astype(np.int32)).to(dev)
        mixed = int(chosen.sum())
        ops.mixup_into(mel, labels, partner, lam, out, targets)              # the checked call once; then the C entry with its arguments prepared
        args = (ops._ptr(mel), ops._ptr(out), B, T, ops._ptr(labels), ops._ptr(partner), ops._ptr(lam), ops._ptr(targets), ops._stream())
        fn = (lambda args=args, keep=(partner, lam): nat.check(nat.lib.ww_mixup_f32(*args)))
        variants[name] = (fn, 2 * batch_bytes + mixed * (batch_bytes // B), mixed)
    us = {name: [] for name in variants}
    for w in range(windows + 1):                                            # window 0 warms up every variant
        for name, (fn, _, _) in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            torch.cuda.synchronize()
            if w:
                us[name].append(1e3 * a.elapsed_time(b) / launches)
    row = {"B": B, "T": T, "batch_bytes": batch_bytes, "launches_per_window": launches, "windows": windows}
    for name, (_, nbytes, mixed) in variants.items():
        s = spread(us[name])
        row[name] = {"us_per_call": s, "bytes_moved": nbytes, "mixed_rows": mixed, "GB_per_s_at_median": nbytes / s["median"] * 1e-3}
    for name in ("mixup_prob_0.5", "mixup_prob_1.0"):
        row[f"{name}_over_copy_time"] = row[name]["us_per_call"]["median"] / row["copy"]["us_per_call"]["median"]
        row[f"{name}_over_copy_bytes"] = row[name]["bytes_moved"] / row["copy"]["bytes_moved"]
    return row


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def bench_step(dev, windows, min_steps=20, window_ms=300.0, warmup=5):
    rows = []
    for name, cls in (("SimpleWakewordModel", pkg.SimpleWakewordModel), ("WakewordModel", pkg.WakewordModel)):
        for B in (16, 4096):
            torch.manual_seed(0)
            data = -40.0 + 20.0 * torch.randn(B, 1, 80, 32, device=dev)
            hard = torch.randint(0, 2, (B, 1), device=dev)
            u = torch.rand(B, device=dev)
            soft = torch.stack([1.0 - u, u], dim=1).contiguous()
            m_int, m_soft = cls().to(dev).train(), cls().to(dev).train()
            m_soft.load_state_dict(m_int.state_dict())
            t_int, t_soft = pkg.WakewordTrainer(m_int, dev), pkg.WakewordTrainer(m_soft, dev)
            f_int = lambda: t_int.step(data, hard)                                          # noqa: E731
            f_soft = lambda: t_soft.step(data, soft)                                        # noqa: E731
            for fn in (f_int, f_soft):
                window(fn, warmup)
            steps = max(min_steps, int(window_ms / max(window(f_int, warmup), window(f_soft, warmup))) + 1)
            ms_int, ms_soft = [], []
            for _ in range(windows):                                                        # alternating windows
                ms_int.append(window(f_int, steps))
                ms_soft.append(window(f_soft, steps))
            row = {"model": name, "batch": B, "frames": 32, "steps_per_window": steps, "windows": windows,
                   "integer_labels_ms": spread(ms_int), "soft_targets_ms": spread(ms_soft),
                   "soft_over_integer": statistics.median(ms_soft) / statistics.median(ms_int), "train_math": ops.get_train_math()}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del t_int, t_soft, m_int, m_soft
            torch.cuda.empty_cache()
    return rows


def bench_loader(dev, clips, epochs, batch=64):
    proc = pkg.AudioProcessor(device=dev)
    bank = pkg.ClipBank(proc)
    pcm = pkg.synth.make_clips_tiled(0, clips, unique=64)
    bank.add_pcm(pcm[: clips // 2], 1)
    bank.add_pcm(pcm[clips // 2:], 0)
    loader = bank.loader(batch, shuffle=True, augment=True)

    def epoch(config):
        proc.set_mixup(config)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for data, target in loader:
            n += data.shape[0]
        torch.cuda.synchronize()
        assert n == clips and target.dtype == (torch.int64 if config is None else torch.float32)
        return (time.perf_counter() - t0) * 1e3
    random.seed(0)
    torch.manual_seed(0)
    for config in (None, MixupConfig):                                      # one warm-up epoch each
        epoch(config)
    off, on = [], []
    for _ in range(epochs):                                                 # alternating epochs
        off.append(epoch(None))
        on.append(epoch(MixupConfig))
    return {"clips": clips, "batch": batch, "frames": 32, "augment": True, "epochs": epochs, "mixup_off_ms_per_epoch": spread(off),
            "mixup_on_ms_per_epoch": spread(on), "on_over_off": statistics.median(on) / statistics.median(off),
            "mixup_config": {"PROB": MixupConfig.PROB, "ALPHA": MixupConfig.ALPHA, "DOMINANT": MixupConfig.DOMINANT}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mixup_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixup.py measures on the MI355X: no GPU is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"device": pkg._native.device_info(), "torch": torch.__version__,
           "what": "median (min .. max) over alternating windows after a warm-up of every shape; kernel: device events around back-to-back "
                   "calls; step and loader: a host clock around work that ends in a synchronise"}
    out["kernel"] = bench_kernel(dev, a.launches, a.windows)
    print(json.dumps(out["kernel"]), flush=True)
    out["step"] = bench_step(dev, a.windows)
    out["loader"] = bench_loader(dev, a.clips, a.epochs)
    print(json.dumps(out["loader"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
