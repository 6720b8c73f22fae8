#!/usr/bin/env python3
"""What a clip ledger costs: ms per WakewordTrainer.step with and without a ledger, and the update launch alone.

    PYTHONPATH=. python scripts/bench_ledger.py [--steps 20] [--windows 7] [--window-ms 300] [--launches 200] [--out profiles/ledger_bench.json]

step: SimpleWakewordModel, T = 32, B = 16 and B = 4096.  Two trainers on their own copy of the model in this one process, one with a
ClipLedger of 65536 entries and one without -- the run without is the code path the step always had, the baseline -- alternating, after
a warm-up of every shape, in windows of at least `--steps` steps and `--window-ms` that end in a synchronise; median over `--windows`
windows with their spread.  The step with a ledger is `step(data, target, entries=<host int64 array>)`, what train_epoch calls with a
loader's `last_entries`: it pays the pinned upload of the entries and the update launch.
launch: ww_clip_ledger_update_f32 alone at n = 16 and n = 4096, the C entry point with its arguments prepared once, one device-event pair
around `--launches` back-to-back calls per window: rows spread over 65536 entries (a permutation: no two rows share a record), rows
drawn with repetition over 64 entries, and ALL rows on one entry -- the worst case of contention on a record.  Beside it, under the same
clocks, ww_clip_metrics_update_f32 (what `validate` already pays per batch) and ClipLedger.update with host entries (launch plus upload)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import wakeword_jupyterlab_amd as pkg  # noqa: E402
from wakeword_jupyterlab_amd import _native as nat  # noqa: E402
from wakeword_jupyterlab_amd import ops  # noqa: E402
from wakeword_jupyterlab_amd.ledger import ClipLedger  # noqa: E402

N_ENTRIES = 65536


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def measure_steps(a, dev):
    rows = []
    for B in (16, 4096):
        torch.manual_seed(0)
        data = -40.0 + 20.0 * torch.randn(B, 1, 80, 32, device=dev)
        target = torch.randint(0, 2, (B, 1), device=dev)
        entries = np.random.default_rng(B).integers(0, N_ENTRIES, B).astype(np.int64)
        m_plain, m_led = pkg.SimpleWakewordModel().to(dev).train(), pkg.SimpleWakewordModel().to(dev).train()
        m_led.load_state_dict(m_plain.state_dict())
        plain_tr = pkg.WakewordTrainer(m_plain, dev)
        ledger = ClipLedger(N_ENTRIES, dev)
        ledger.begin_epoch()
        led_tr = pkg.WakewordTrainer(m_led, dev, ledger=ledger)
        plain = lambda: plain_tr.step(data, target)                                         # noqa: E731
        with_ledger = lambda: led_tr.step(data, target, entries=entries)                    # noqa: E731
        for fn in (plain, with_ledger):
            window(fn, a.warmup)
        steps = max(a.steps, int(a.window_ms / max(window(plain, a.warmup), window(with_ledger, a.warmup))) + 1)
        t_plain, t_led = [], []
        for _ in range(a.windows):                                                          # alternating windows
            t_plain.append(window(plain, steps))
            t_led.append(window(with_ledger, steps))
        head = ledger.read().header
        assert head["rows"] == B * head["updates"] and head["bad_entries"] == head["skipped"] == 0
        row = {"model": "SimpleWakewordModel", "batch": B, "frames": 32, "steps_per_window": steps, "windows": a.windows,
               "step_ms": spread(t_plain), "step_with_ledger_ms": spread(t_led),
               "ratio_with_over_without": statistics.median(t_led) / statistics.median(t_plain),
               "added_us_per_step": 1e3 * (statistics.median(t_led) - statistics.median(t_plain)),
               "ranges_overlap": not (max(t_plain) < min(t_led) or max(t_led) < min(t_plain)),
               "ledger_updates_counted": head["updates"], "train_math": ops.get_train_math()}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del plain_tr, led_tr, m_plain, m_led, ledger
        torch.cuda.empty_cache()
    return rows


def event_windows(call, launches, windows):
    us = []
    for w in range(windows + 1):                                                            # window 0 warms up
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(launches):
            call()
        e.record()
        torch.cuda.synchronize()
        if w:
            us.append(1e3 * s.elapsed_time(e) / launches)
    return spread(us)


def measure_launch(a, dev):
    rows = []
    g = torch.Generator().manual_seed(0)
    for n in (16, 4096):
        z = (torch.randn(n, 2, generator=g) * 6.0).to(dev)
        y = (torch.rand(n, generator=g) < 0.3).to(torch.int64).to(dev)
        rng = np.random.default_rng(n)
        cases = {"spread_over_65536_entries": rng.permutation(N_ENTRIES)[:n], "repeats_over_64_entries": rng.integers(0, 64, n),
                 "all_rows_one_entry": np.full(n, 7)}
        row = {"n": n, "launches_per_window": a.launches, "windows": a.windows}
        for name, host in cases.items():
            host = host.astype(np.int64)
            e = torch.from_numpy(host).to(dev)
            state = ops.new_clip_ledger(dev, N_ENTRIES)
            args = (ops._ptr(z), ops._ptr(y), ops._ptr(e), n, 3, ops._ptr(state.buffer), N_ENTRIES, ops._stream())
            row[name + "_us_per_call"] = event_windows(lambda: nat.lib.ww_clip_ledger_update_f32(*args), a.launches, a.windows)
            rep = ops.read_clip_ledger(state)
            assert rep.header["updates"] == a.launches * (a.windows + 1) and int(rep.seen.sum()) == n * rep.header["updates"]
            if name == "all_rows_one_entry":
                assert rep.seen[7] == n * rep.header["updates"]
        ledger = ClipLedger(N_ENTRIES, dev)
        host = cases["spread_over_65536_entries"].astype(np.int64)
        row["ClipLedger_update_host_entries_us_per_call"] = event_windows(lambda: ledger.update(host, z, y), a.launches, a.windows)
        metrics = ops.new_clip_metrics(dev, (0.8,))
        margs = (ops._ptr(z), ops._ptr(y), n, ops._ptr(metrics.buffer), ops._stream())
        row["clip_metrics_update_us_per_call"] = event_windows(lambda: nat.lib.ww_clip_metrics_update_f32(*margs), a.launches, a.windows)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ledger_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ledger.py measures on the MI355X: no GPU is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"device": nat.device_info(), "torch": torch.__version__,
           "what": "ms per WakewordTrainer.step without (the baseline) and with a ClipLedger, median over alternating windows that end in a "
                   "synchronise; us per ww_clip_ledger_update_f32 call from device events around back-to-back calls",
           "step": measure_steps(a, dev), "launch": measure_launch(a, dev)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
