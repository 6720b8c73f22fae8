#!/usr/bin/env python3
"""What loss-ranked selection costs on the MI355X, three measurements in one process:

  select   ww_hard_select_f32 (integer labels with class weights, keep = n / 4, keep_class 1, scores and stats written) beside
           ww_ce_loss_ex_f32 on the same logits and labels -- a latency yardstick: one workgroup each -- at n = 16, 4096 and 65536
  gather   ww_select_rows_f32 at (n, k) = (4096, 1024), T = 32 (data, labels, entries) beside a device-to-device copy_ of the same
           1024 rows: the bytes a gather has to move
           both: device events around `--launches` back-to-back calls per window, the variants alternating window by window after a
           warm-up window each; microseconds per call
  step     WakewordTrainer.step at B = 4096, T = 32 for both model classes: select off, and HardSelect(keep, keep_class=1) with keep in
           {2048, 1024, 512}; beside them the plain step (select=None, the native calls the step issued before selection existed) at
           B = 2048, 1024 and 512 -- what the k-row part of a mined step costs on its own.  Every variant on its own copy of the model,
           alternating windows that end in a synchronise; milliseconds per step.  mined(k) - plain(k) is what scoring, selecting and
           gathering add; mined(k) against plain(4096) says whether mining pays for itself in time at this batch size.

Every figure is the median over the windows with their spread (min .. max).  Writes profiles/select_bench.json.

    PYTHONPATH=. python scripts/bench_select.py [--launches 200] [--windows 7] [--out profiles/select_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import wakeword_jupyterlab_amd as pkg  # noqa: E402
from wakeword_jupyterlab_amd import _native as nat  # noqa: E402
from wakeword_jupyterlab_amd import ops  # noqa: E402


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def event_windows(variants, launches, windows):
    """{name: [us per call per window]}: window 0 warms up every variant."""
    us = {name: [] for name in variants}
    for w in range(windows + 1):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            torch.cuda.synchronize()
            if w:
                us[name].append(1e3 * a.elapsed_time(b) / launches)
    return us


def bench_select(dev, launches, windows):
    rows = []
    for n in (16, 4096, 65536):
        g = torch.Generator().manual_seed(n)
        z = (4.0 * torch.randn(n, 2, generator=g)).to(dev)
        y = (torch.rand(n, generator=g) < 0.05).to(torch.int64).to(dev)
        keep = max(1, n // 4)
        d, loss, stats = torch.empty_like(z), torch.empty((), device=dev), ops.new_loss_stats(dev)
        sel, scores, sstats = torch.empty(keep, device=dev, dtype=torch.int64), torch.empty(n, device=dev, dtype=torch.float64), ops.new_select_stats(dev)
        ws = torch.empty(ops.hard_select_workspace_bytes(n), device=dev, dtype=torch.uint8)
        opts = ops.loss_opts(weight=(1.0, 7.5))
        ops.ce_loss_into(z, y, d, loss, stats, opts=opts)                        # the checked calls once; then the C entries with prepared arguments
        ops.hard_select_into(z, y, keep, sel, scores, sstats, ws, opts=opts, keep_class=1)
        stream = ops._stream()
        ce_args = (ops._ptr(z), ops._ptr(y), n, C.byref(opts), ops._ptr(d), ops._ptr(loss), ops._ptr(stats), stream)
        hs_args = (ops._ptr(z), ops._ptr(y), nat.TARGET_LABELS, n, keep, C.byref(opts), 1, ops._ptr(sel), ops._ptr(scores), ops._ptr(sstats),
                   ops._ptr(ws), stream)
        us = event_windows({"ce_loss_ex": lambda a=ce_args: nat.check(nat.lib.ww_ce_loss_ex_f32(*a)),
                            "hard_select": lambda a=hs_args: nat.check(nat.lib.ww_hard_select_f32(*a))}, launches, windows)
        row = {"n": n, "keep": keep, "launches_per_window": launches, "windows": windows, "ce_loss_ex_us": spread(us["ce_loss_ex"]),
               "hard_select_us": spread(us["hard_select"]),
               "hard_select_over_ce_time": statistics.median(us["hard_select"]) / statistics.median(us["ce_loss_ex"])}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def bench_gather(dev, launches, windows, n=4096, k=1024, T=32):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n, 1, 80, T, generator=g).to(dev)
    y = torch.randint(0, 2, (n,), generator=g).to(dev)
    entries = torch.arange(n, device=dev)
    sel = torch.sort(torch.randperm(n, generator=g)[:k]).values.to(dev)
    gx, gy, ge = torch.empty(k, 1, 80, T, device=dev), torch.empty(k, device=dev, dtype=torch.int64), torch.empty(k, device=dev, dtype=torch.int64)
    ops.select_rows_into(x, sel, gx, y, gy, entries, ge)
    assert torch.equal(gx, x[sel]) and torch.equal(gy, y[sel]) and torch.equal(ge, sel)
    args = (ops._ptr(x), n, T, ops._ptr(sel), k, ops._ptr(gx), ops._ptr(y), nat.TARGET_LABELS, ops._ptr(gy), ops._ptr(entries), ops._ptr(ge),
            None, None, ops._stream())
    src = x[:k]
    us = event_windows({"select_rows": lambda: nat.check(nat.lib.ww_select_rows_f32(*args)), "copy": lambda: gx.copy_(src)}, launches, windows)
    row = {"n": n, "k": k, "frames": T, "bytes_moved": 2 * k * 80 * T * 4, "launches_per_window": launches, "windows": windows,
           "select_rows_us": spread(us["select_rows"]), "device_copy_us": spread(us["copy"]),
           "select_rows_over_copy_time": statistics.median(us["select_rows"]) / statistics.median(us["copy"])}
    print(json.dumps(row), flush=True)
    return row


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def bench_step(dev, windows, B=4096, keeps=(2048, 1024, 512), min_steps=10, window_ms=300.0, warmup=3):
    classes = {"SimpleWakewordModel": pkg.SimpleWakewordModel, "WakewordModel": pkg.WakewordModel}
    rows = []
    for name, cls in classes.items():
        torch.manual_seed(0)
        data = -40.0 + 20.0 * torch.randn(B, 1, 80, 32, device=dev)
        y = (torch.rand(B, device=dev) < 0.05).to(torch.int64)
        first = cls().to(dev).train()
        fns = {}

        def add(tag, select, rows_):
            m = cls().to(dev).train()
            m.load_state_dict(first.state_dict())
            t = pkg.WakewordTrainer(m, dev, select=select)
            xs, ys = data[:rows_].contiguous(), y[:rows_].contiguous()
            fns[tag] = lambda: t.step(xs, ys)
        add(f"plain_B{B}", None, B)
        for k in keeps:
            add(f"mined_keep{k}", pkg.HardSelect(k, keep_class=1), B)
            add(f"plain_B{k}", None, k)
        for fn in fns.values():
            window(fn, warmup)
        steps = max(min_steps, int(window_ms / max(window(fn, warmup) for fn in fns.values())) + 1)
        ms = {tag: [] for tag in fns}
        for _ in range(windows):                                                            # alternating windows
            for tag, fn in fns.items():
                ms[tag].append(window(fn, steps))
        med = {tag: statistics.median(v) for tag, v in ms.items()}
        row = {"model": name, "batch": B, "frames": 32, "steps_per_window": steps, "windows": windows, "train_math": ops.get_train_math(),
               "ms": {tag: spread(v) for tag, v in ms.items()},
               "mined_minus_plain_at_keep_ms": {str(k): med[f"mined_keep{k}"] - med[f"plain_B{k}"] for k in keeps},
               "mined_over_plain_full_batch": {str(k): med[f"mined_keep{k}"] / med[f"plain_B{B}"] for k in keeps}}
        rows.append(row)
        print(json.dumps(row), flush=True)
        fns.clear()
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "select_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_select.py measures on the MI355X: no GPU is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"device": nat.device_info(), "torch": torch.__version__,
           "what": "median (min .. max) over alternating windows after a warm-up of every variant; select and gather: device events around "
                   "back-to-back calls; step: a host clock around work that ends in a synchronise.  plain_B* is this tree's step with "
                   "select=None, which issues the native calls the step issued before selection existed; a build of the parent commit "
                   "was not timed in this run."}
    out["select"] = bench_select(dev, a.launches, a.windows)
    out["gather"] = bench_gather(dev, a.launches, a.windows)
    out["step"] = bench_step(dev, a.windows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
