#!/usr/bin/env python3
"""ClipBank: the gather kernel against a device-to-device copy of the same bytes, the peak kernel over one
hour of audio split two ways, and whole epochs of the bank loader against the file loader.

    PYTHONPATH=. python scripts/bench_bank.py [--batch 4096] [--calls 60] [--files 8192] [--rounds 3] [--out profiles/bank_bench.json]

gather: B x 16000 samples per call, each normalisation, from 1 s entries at start 0 and from 3 s entries at random starts (all four source
alignments); device events around every call, a torch `copy_` of the same 2 * 4 * B * N bytes alternating with it call for call.
peaks: one segment of one hour as a single entry and as 12,000 entries of 0.3 s.
epochs: `--files` synthetic 1 s files in a temporary directory, `ds.loader(B)` and `ds.cache().loader(B)` alternating epoch for epoch
after one warm-up epoch each, augmentation off and on; wall seconds and host CPU seconds (time.process_time) per epoch."""
import argparse
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
from wakeword_jupyterlab_amd import bank as bankmod  # noqa: E402

N = 16000
HBM_PEAK = 8.0e12          # bytes/s, the card's specified peak


def _timed_pairs(fns, calls):
    """Each function `calls` times, alternating call for call, a device event pair around every call -> ms lists."""
    ms = [[] for _ in fns]
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(calls):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            pairs.append((k, a, b))
    torch.cuda.synchronize()
    for k, a, b in pairs:
        ms[k].append(a.elapsed_time(b))
    return ms


def measure_gather(batch, calls, dev):
    proc = pkg.AudioProcessor(device=dev)
    rng = np.random.default_rng(0)
    out = torch.empty((batch, N), device=dev)
    src = torch.randn((batch, N), device=dev)
    nbytes = 2 * 4 * batch * N
    res = []
    for name, seconds in (("1 s entries, start 0", 1), ("3 s entries, random starts", 3)):
        b = pkg.ClipBank(proc)
        b.add_buffer(torch.randn(batch * seconds * N, device=dev), np.full(batch, seconds * N))
        entries = np.arange(batch, dtype=np.int64)
        starts = np.zeros(batch, np.int64) if seconds == 1 else rng.integers(0, (seconds - 1) * N + 1, size=batch)
        for norm in (None, "entry", "window"):
            norms = np.full(batch, bankmod.NORMS[norm], np.int32)
            g, c = _timed_pairs([lambda: b._gather(entries, starts, norms, out), lambda: out.copy_(src)], calls)
            mg, mc = statistics.median(g), statistics.median(c)
            res.append({"case": name, "normalize": norm or "none", "batch": batch, "n_samples": N, "calls": calls, "bytes_per_call": nbytes,
                        "start_alignments": np.bincount(starts % 4, minlength=4).tolist(),
                        "gather_ms_median": mg, "gather_ms_mean": statistics.fmean(g), "gather_ms_min": min(g),
                        "copy_ms_median": mc, "copy_ms_mean": statistics.fmean(c), "copy_ms_min": min(c),
                        "gather_over_copy": mg / mc, "gather_bytes_per_s": nbytes / (mg * 1e-3), "copy_bytes_per_s": nbytes / (mc * 1e-3),
                        "gather_share_of_hbm_peak": nbytes / (mg * 1e-3) / HBM_PEAK, "copy_share_of_hbm_peak": nbytes / (mc * 1e-3) / HBM_PEAK})
        del b
    return res


def measure_peaks(calls, dev):
    total = 3600 * N
    data = torch.randn(total, device=dev)
    one = torch.tensor([0, total], device=dev)
    many = torch.arange(0, total + 1, 4800, device=dev)
    assert many.numel() == 12001
    t1, t2 = _timed_pairs([lambda: bankmod.bank_peaks(data, one), lambda: bankmod.bank_peaks(data, many)], calls)
    assert float(bankmod.bank_peaks(data, one)[0]) == float(bankmod.bank_peaks(data, many).max()) == float(data.abs().max())
    return [{"entries": n, "samples": total, "calls": calls, "ms_median": statistics.median(t), "ms_min": min(t),
             "bytes_per_s": 4 * total / (statistics.median(t) * 1e-3), "share_of_hbm_peak": 4 * total / (statistics.median(t) * 1e-3) / HBM_PEAK}
            for n, t in ((1, t1), (12000, t2))]


def measure_epochs(files, batch, rounds, dev):
    import struct
    clips = pkg.synth.make_clips_tiled(0, files, unique=64, n=N)
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i in range(files):
            raw = np.clip(np.round(clips[i] * 30000), -32768, 32767).astype("<i2").tobytes()
            hdr = (b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, N, 2 * N, 2, 16) +
                   b"data" + struct.pack("<I", len(raw)))
            paths.append(os.path.join(d, f"clip_{i:05d}.wav"))
            with open(paths[-1], "wb") as f:
                f.write(hdr + raw)
        proc = pkg.AudioProcessor(device=dev)
        out = {"files": files, "batch": batch, "rounds": rounds}
        for augment in (False, True):
            ds = pkg.WakewordDataset(paths[: files // 2], paths[files // 2:], proc, augment=augment, verbose=False)
            bank = ds.cache()
            loaders = {"file": ds.loader(batch, shuffle=True), "bank": bank.loader(batch, shuffle=True, augment=augment)}

            def epoch(ld):
                torch.cuda.synchronize()
                w0, c0 = time.perf_counter(), time.process_time()
                n = 0
                for data, _ in ld:
                    n += data.shape[0]
                torch.cuda.synchronize()
                assert n == files
                return time.perf_counter() - w0, time.process_time() - c0
            random.seed(0)
            torch.manual_seed(0)
            for ld in loaders.values():
                epoch(ld)                                                   # warm-up
            wall = {k: [] for k in loaders}
            cpu = {k: [] for k in loaders}
            for _ in range(rounds):
                for k, ld in loaders.items():                               # alternating epoch for epoch
                    w, c = epoch(ld)
                    wall[k].append(w)
                    cpu[k].append(c)
            key = "augment_on" if augment else "augment_off"
            out[key] = {k: {"epoch_s_median": statistics.median(wall[k]), "epoch_s_all": wall[k], "clips_per_s": files / statistics.median(wall[k]),
                            "host_cpu_s_median": statistics.median(cpu[k]), "host_cpu_s_all": cpu[k]} for k in loaders}
            out[key]["bank_over_file"] = out[key]["bank"]["epoch_s_median"] / out[key]["file"]["epoch_s_median"]
            out["bank_build"] = dict(bank.stats, bank_bytes=bank.nbytes)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--files", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result JSON here")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"device": nat.device_info(), "hbm_peak_bytes_per_s": HBM_PEAK, "gather": measure_gather(a.batch, a.calls, dev),
           "peaks": measure_peaks(max(10, a.calls // 3), dev), "epochs": measure_epochs(a.files, a.batch, a.rounds, dev)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
