#!/usr/bin/env python3
"""Microphone-channel augmentation: the channel kernel alone, beside a device-to-device copy of the same
bytes and beside the augmentation chain (KA) on the same batch, and what switching it on costs an augmented epoch of the bank loader.

    PYTHONPATH=. python scripts/bench_channel.py [--batch 4096] [--launches 50] [--windows 9] [--files 8192] [--rounds 5]
                                                 [--out profiles/channel_bench.json]

kernel: B x N at N = 16000 and 8000, the default config (records drawn on the device from one seed) and records with all 8 sections and
the saturator on, out of place from a source that is never written (`--launches` back-to-back calls of the C entry point per window)
and in place as the loaders call it (10 calls per window, the batch restored before every window; see measure_kernel).
scripts/bench_specaug.py's method: one device-event pair around the calls of a window, `--windows` windows after a warm-up window; the
median window gives the time per call.  In the same run and by the same method: `copy_` of the batch into a second buffer (the same
bytes read and written once), and KA on the same batch: ww_augment_rir_f32 itself with its plan array and workspace built once (what
ops.augment calls), and ops.augment with the same array for comparison (`--launches` / 10 calls per window: it is the longer call).
The share of clips touched is read back once through ops.channel_records.
wrapper: host time per AudioProcessor.channel_effects_batch call on a one-clip batch.
loader: scripts/bench_bank.py's augmented epoch (`--files` synthetic 1 s clips in a ClipBank, batch `--batch`, shuffle, augment=True),
epochs with processor.set_channel_effects(None) and (ChannelConfig) alternating in one run after a warm-up epoch each; wall seconds per
epoch, their spread, and the parent commit's figure from profiles/bank_bench.json."""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import wakeword_jupyterlab_amd as pkg  # noqa: E402
from wakeword_jupyterlab_amd import _native as nat  # noqa: E402
from wakeword_jupyterlab_amd import ops  # noqa: E402
from wakeword_jupyterlab_amd.config import AudioConfig, ChannelConfig  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_PLACE_LAUNCHES = 10
ALL_ON = {"highpass": 20.0, "low_shelf": (150.0, 5.0), "peaks": [(100.0, 6.0, 4.0), (700.0, -4.0, 1.0), (2200.0, 5.0, 0.7), (5000.0, -6.0, 2.0)],
          "high_shelf": (3000.0, -5.0), "lowpass": 3400.0, "drive": 2.0}


def windows_of(fn, launches, windows, before_window=None):
    """µs per call of every window after the warm-up one: a device-event pair around `launches` back-to-back calls.  `before_window`
    runs outside the events (it restores the data an in-place call has changed)."""
    ms = []
    for w in range(windows + 1):
        if before_window is not None:
            before_window()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        if w:
            ms.append(a.elapsed_time(b) / launches)
    return {"us_per_call_median": 1e3 * statistics.median(ms), "us_per_call_min": 1e3 * min(ms), "us_per_call_max": 1e3 * max(ms),
            "launches_per_window": launches, "windows": windows}


def measure_kernel(batch, launches, windows, dev):
    """Every timed launch filters finite audio.  Out of place the source is never written, so each launch does the same work on the same
    data.  In place (what the loaders do: clips whose record is "off" are skipped) a launch filters the previous launch's output, which
    a cascade with gain lets grow by up to some 30 dB per launch: the batch is restored from the source before every window, outside
    the events, a window is IN_PLACE_LAUNCHES launches (at most 300 dB of the 770 dB float32 holds), and the batch is asserted
    finite and not all zero after every window."""
    res = []
    for N in (16000, 8000):
        src = 2.0 * torch.rand((batch, N), device=dev) - 1.0
        keep = src.clone()
        pcm, other = src.clone(), torch.empty_like(src)
        seed = 0x5EED0000 + N
        g = ops._channel_struct(ChannelConfig)
        drawn = ops.channel_records(seed, batch, device=dev)
        rec_np = drawn.cpu().numpy()
        sections = rec_np[:, :40].reshape(batch, 8, 5)
        identity = (sections[:, :, 0] == 1) & (sections[:, :, 1:] == 0).all(axis=2)
        touched = ~(identity.all(axis=1) & (rec_np[:, 40] == 0))
        all_on = torch.from_numpy(np.repeat(ops.pack_channel_plans([ALL_ON]), batch, axis=0)).to(dev)
        stream = ops._stream()

        def args(dst, records):
            if records is None:
                return (ops._ptr(src if dst is other else dst), ops._ptr(dst), batch, N, N, None, seed, C.byref(g), stream)
            return (ops._ptr(src if dst is other else dst), ops._ptr(dst), batch, N, N, ops._ptr(records), 0, None, stream)

        def restore():
            assert bool(torch.isfinite(pcm).all()) and bool((pcm != 0).any()), "an in-place window left non-finite or all-zero audio"
            pcm.copy_(src)

        nat.check(nat.lib.ww_channel_f32(*args(pcm, None)))
        assert torch.equal(pcm, ops.channel_effects(src, seed=seed))            # the raw call is the wrapper's launch
        entry = {"n_samples": N, "batch": batch, "bytes_read_plus_written": 2 * 4 * batch * N, "share_of_clips_touched": float(touched.mean()),
                 "sections_on_per_touched_clip": float((~identity)[touched].sum(axis=1).mean()),
                 "share_of_clips_with_drive": float((rec_np[:, 40] != 0).mean())}
        for name, records in (("default_config", None), ("all_sections_on", all_on)):
            a = args(other, records)
            entry[name + "_out_of_place"] = windows_of(lambda: nat.lib.ww_channel_f32(*a), launches, windows)
            assert bool(torch.isfinite(other).all()) and torch.equal(src, keep)
            a = args(pcm, records)
            entry[name + "_in_place"] = windows_of(lambda: nat.lib.ww_channel_f32(*a), IN_PLACE_LAUNCHES, windows, before_window=restore)
            restore()
        entry["device_copy"] = windows_of(lambda: other.copy_(src), launches, windows)
        # KA: ww_augment_rir_f32 itself (what ops.augment calls for every batch), its plan array, "no reverb" array and workspace built once
        proc = pkg.AudioProcessor(type("Cfg", (AudioConfig,), {"DURATION": N / 16000.0}), device=dev)
        random.seed(N)
        plans = ops._plans_array([proc.draw_augment_plan(length=N) for _ in range(batch)], batch)
        rir = ops._rir_array((), None, batch)
        ws = torch.empty(nat.check(nat.lib.ww_augment_rir_workspace_bytes(batch, N)), device=dev, dtype=torch.uint8)
        ka = (ops._ptr(src), batch, N, N, plans, None, None, 0, rir, None, 0, ops._ptr(other), N, ops._ptr(ws), stream)
        nat.check(nat.lib.ww_augment_rir_f32(*ka))
        assert torch.equal(other, ops.augment(src, plans))
        entry["augment_ka"] = windows_of(lambda: nat.lib.ww_augment_rir_f32(*ka), max(1, launches // 10), windows)
        entry["augment_ka_wrapper"] = windows_of(lambda: ops.augment(src, plans), max(1, launches // 10), windows)
        assert torch.equal(src, keep)
        for name in ("default_config_in_place", "default_config_out_of_place"):
            entry[name + "_over_copy"] = entry[name]["us_per_call_median"] / entry["device_copy"]["us_per_call_median"]
            entry[name + "_over_ka"] = entry[name]["us_per_call_median"] / entry["augment_ka"]["us_per_call_median"]
        res.append(entry)
    return res


def measure_wrapper_host(dev, calls=300):
    """Host microseconds per AudioProcessor.channel_effects_batch call (config struct, checks, launch): a one-clip batch, so that the
    kernel is short and the launches never queue up; the host clock around `calls` calls without a synchronise between them."""
    proc = pkg.AudioProcessor(device=dev)
    proc.set_channel_effects(ChannelConfig)
    pcm = torch.zeros((1, 16000), device=dev)
    us = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(calls):
            proc.channel_effects_batch(pcm, seed=i, inplace=True)
        us.append(1e6 * (time.perf_counter() - t0) / calls)
        torch.cuda.synchronize()
    return {"calls": calls, "host_us_per_call_median": statistics.median(us[1:]), "host_us_per_call_all": us[1:]}


def measure_loader(files, batch, rounds, dev):
    import tempfile
    proc = pkg.AudioProcessor(device=dev)
    clips = pkg.synth.make_clips_tiled(0, files, unique=64, n=16000)
    with tempfile.TemporaryDirectory() as d:                                # the files of bench_bank.py's epochs, decoded once into the bank
        paths = [os.path.join(d, f"clip_{i:05d}.wav") for i in range(files)]
        for path, clip in zip(paths, clips):
            pkg.synth.write_wav16(path, clip)
        bank = pkg.WakewordDataset(paths[: files // 2], paths[files // 2:], proc, augment=True, verbose=False).cache()
    loader = bank.loader(batch, shuffle=True, augment=True)

    def epoch(config):
        proc.set_channel_effects(config)
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
    configs = {"unset": None, "set": ChannelConfig}
    for c in configs.values():
        epoch(c)                                                            # warm-up
    wall = {k: [] for k in configs}
    for _ in range(rounds):
        for k, c in configs.items():                                        # alternating epoch for epoch
            wall[k].append(epoch(c))
    proc.set_channel_effects(None)
    out = {"files": files, "batch": batch, "rounds": rounds, "batches_per_epoch": len(loader)}
    for k in configs:
        out[k] = {"epoch_s_median": statistics.median(wall[k]), "epoch_s_min": min(wall[k]), "epoch_s_max": max(wall[k]), "epoch_s_all": wall[k],
                  "clips_per_s": files / statistics.median(wall[k])}
    out["set_minus_unset_s_per_batch"] = (out["set"]["epoch_s_median"] - out["unset"]["epoch_s_median"]) / len(loader)
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
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--files", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the result JSON here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_channel.py measures on the MI355X: no GPU is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"device": nat.device_info(), "kernel": measure_kernel(a.batch, a.launches, a.windows, dev),
           "wrapper_host": measure_wrapper_host(dev), "loader": measure_loader(a.files, a.batch, a.rounds, dev)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
