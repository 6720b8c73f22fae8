#!/usr/bin/env python3
"""SpecAugment: the masking kernel alone, and what switching it on costs an augmented epoch of the bank loader.

    PYTHONPATH=. python scripts/bench_specaug.py [--batch 4096] [--launches 200] [--windows 9] [--files 8192] [--rounds 7]
                                                 [--out profiles/specaug_bench.json]

kernel: B x [80, T] at T = 32 and 63, in place, each fill mode, records drawn on the device from one seed.  One device-event pair around
`--launches` back-to-back calls per window, `--windows` windows after a warm-up window; the median window gives the time per call.
Bytes per call are computed from the shapes and the records (read back once through ops.spec_augment_records): every clip with a mask is
read once for the mean and the minimum (320 T bytes; nothing under a constant fill), and every masked float is written once.  A batch
of 4,096 clips is 42 MB at T = 32 and 83 MB at T = 63 and stays in the 256 MiB last-level cache between calls, so bytes/s over the HBM
peak says how the kernel compares with the slowest memory it could be reading, not that it reads HBM.
loader: scripts/bench_bank.py's augmented epoch (`--files` synthetic 1 s clips in a ClipBank, batch `--batch`, shuffle, augment=True),
epochs with processor.set_spec_augment(None) and (SpecAugmentConfig) alternating in one run after a warm-up epoch each; wall seconds per
epoch, their spread, and the parent commit's figure from profiles/bank_bench.json."""
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
from wakeword_jupyterlab_amd.config import SpecAugmentConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 16000
HBM_PEAK = 8.0e12          # bytes/s, the card's specified peak (scripts/bench_bank.py uses the same)


def masked_counts(records: np.ndarray, T: int) -> np.ndarray:
    """Masked positions per clip from int16 records [B, 16]: |rows| T + |cols| (80 - |rows|)."""
    rec = records.astype(np.int64)
    rows = np.zeros((rec.shape[0], 80), bool)
    cols = np.zeros((rec.shape[0], T), bool)
    for i in range(4):
        rows |= (np.arange(80)[None] >= rec[:, 2 * i, None]) & (np.arange(80)[None] < rec[:, 2 * i, None] + rec[:, 2 * i + 1, None])
        cols |= (np.arange(T)[None] >= rec[:, 8 + 2 * i, None]) & (np.arange(T)[None] < rec[:, 8 + 2 * i, None] + rec[:, 9 + 2 * i, None])
    r, c = rows.sum(1), cols.sum(1)
    return r * T + c * (80 - r)


def measure_kernel(batch, launches, windows, dev):
    res = []
    for T in (32, 63):
        src = -80.0 * torch.rand((batch, 1, 80, T), device=dev)
        seed = 0x5EED0000 + T
        masked = masked_counts(ops.spec_augment_records(seed, batch, T, device=dev).cpu().numpy(), T)
        touched = int((masked > 0).sum())
        for fill in ("mean", "min", -80.0):
            cfg = type("Cfg", (SpecAugmentConfig,), {"FILL": fill})
            mel = src.clone()
            read = 0 if not isinstance(fill, str) else touched * 320 * T
            nbytes = read + 4 * int(masked.sum())
            ms = []
            # the C entry point itself, arguments prepared once: the wrapper's checks cost the host more per call than the kernel runs
            prob, n_freq, freq_max, n_time, time_max, mode, value = ops._spec_args(cfg, T)
            args = (ops._ptr(mel), ops._ptr(mel), batch, T, None, seed, prob, n_freq, freq_max, n_time, time_max, mode, value, ops._stream())
            want = ops.spec_augment(src, seed=seed, config=cfg)
            nat.check(nat.lib.ww_spec_augment_f32(*args))
            assert torch.equal(mel, want)
            for w in range(windows + 1):                                    # window 0 warms up
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(launches):
                    nat.lib.ww_spec_augment_f32(*args)
                b.record()
                torch.cuda.synchronize()
                if w:
                    ms.append(a.elapsed_time(b) / launches)
            med = statistics.median(ms)
            res.append({"T": T, "batch": batch, "fill": fill, "launches_per_window": launches, "windows": windows,
                        "clips_with_a_mask": touched, "masked_floats": int(masked.sum()), "bytes_read": read, "bytes_per_call": nbytes,
                        "ms_per_call_median": med, "ms_per_call_min": min(ms), "ms_per_call_max": max(ms),
                        "bytes_per_s": nbytes / (med * 1e-3), "share_of_hbm_peak": nbytes / (med * 1e-3) / HBM_PEAK})
    return res


def measure_loader(files, batch, rounds, dev):
    import tempfile
    proc = pkg.AudioProcessor(device=dev)
    clips = pkg.synth.make_clips_tiled(0, files, unique=64, n=N)
    with tempfile.TemporaryDirectory() as d:                                # the files of bench_bank.py's epochs, decoded once into the bank
        paths = [os.path.join(d, f"clip_{i:05d}.wav") for i in range(files)]
        for path, clip in zip(paths, clips):
            pkg.synth.write_wav16(path, clip)
        bank = pkg.WakewordDataset(paths[: files // 2], paths[files // 2:], proc, augment=True, verbose=False).cache()
    loader = bank.loader(batch, shuffle=True, augment=True)

    def epoch(config):
        proc.set_spec_augment(config)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for data, _ in loader:
            n += data.shape[0]
        torch.cuda.synchronize()
        assert n == files
        return time.perf_counter() - t0
    random.seed(0)
    torch.manual_seed(0)
    configs = {"off": None, "on": SpecAugmentConfig}
    for c in configs.values():
        epoch(c)                                                            # warm-up
    wall = {k: [] for k in configs}
    for _ in range(rounds):
        for k, c in configs.items():                                        # alternating epoch for epoch
            wall[k].append(epoch(c))
    proc.set_spec_augment(None)
    out = {"files": files, "batch": batch, "rounds": rounds, "batches_per_epoch": len(loader)}
    for k in configs:
        out[k] = {"epoch_s_median": statistics.median(wall[k]), "epoch_s_min": min(wall[k]), "epoch_s_max": max(wall[k]), "epoch_s_all": wall[k],
                  "clips_per_s": files / statistics.median(wall[k])}
    out["on_minus_off_s_per_batch"] = (out["on"]["epoch_s_median"] - out["off"]["epoch_s_median"]) / len(loader)
    out["spread_s_per_batch"] = max(out[k]["epoch_s_max"] - out[k]["epoch_s_min"] for k in configs) / len(loader)
    try:
        with open(os.path.join(ROOT, "profiles", "bank_bench.json")) as f:
            parent = json.load(f)["epochs"]
        out["parent_bank_augment_on"] = {"files": parent["files"], "batch": parent["batch"], **parent["augment_on"]["bank"]}
    except (OSError, KeyError, ValueError):
        out["parent_bank_augment_on"] = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--files", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the result JSON here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_specaug.py measures on the MI355X: no GPU is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"device": nat.device_info(), "hbm_peak_bytes_per_s": HBM_PEAK, "kernel": measure_kernel(a.batch, a.launches, a.windows, dev),
           "loader": measure_loader(a.files, a.batch, a.rounds, dev)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
