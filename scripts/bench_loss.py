#!/usr/bin/env python3
"""The loss for imbalanced data: ww_ce_loss_ex_f32 against ww_ce_loss_f32 in one process, at the batch size of
the training step (n = 16) and at n = 4096, for weighted + smoothed cross-entropy and for the focal loss, and ww_ce_loss_soft_f32 (section
3n) with the weighted + smoothed options on [n, 2] class probabilities.

    PYTHONPATH=. python scripts/bench_loss.py [--launches 500] [--windows 9] [--out profiles/loss_bench.json]

The C entry points themselves with their arguments prepared once; loss, gradient and the stats record all written, as in the step.  One
device-event pair around `--launches` back-to-back calls per window; the four variants alternate window by window after a warm-up
window each; median and range of the windows, in microseconds per call.  Back-to-back calls on one stream serialise on the record, so
this is the time from one call's start to the next one's, launch overhead included -- what a training step pays for its loss."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from wakeword_jupyterlab_amd import _native as nat  # noqa: E402
from wakeword_jupyterlab_amd import ops  # noqa: E402

VARIANTS = {"plain": None, "weighted_smoothed": dict(weight=(0.25, 4.0), label_smoothing=0.125), "focal": dict(weight=(0.25, 4.0), focal_gamma=2.0)}
SOFT = dict(weight=(0.25, 4.0), label_smoothing=0.125)


def measure(n, launches, windows, dev):
    g = torch.Generator().manual_seed(n)
    z = (torch.randn(n, 2, generator=g) * 6.0).to(dev)
    y = (torch.rand(n, generator=g) < 0.1).to(torch.int64).to(dev)
    d, loss, stats = torch.empty_like(z), torch.empty((), device=dev), ops.new_loss_stats(dev)
    stream = ops._stream()
    calls = {}
    for name, kw in VARIANTS.items():
        if kw is None:
            calls[name] = (nat.lib.ww_ce_loss_f32, (ops._ptr(z), ops._ptr(y), n, ops._ptr(d), ops._ptr(loss), ops._ptr(stats), stream), None)
        else:
            opts = ops.loss_opts(**kw)
            calls[name] = (nat.lib.ww_ce_loss_ex_f32, (ops._ptr(z), ops._ptr(y), n, C.byref(opts), ops._ptr(d), ops._ptr(loss), ops._ptr(stats), stream), opts)
    t = torch.stack([1.0 - y.to(torch.float32), y.to(torch.float32)], dim=1).mul_(0.75).add_(0.125).contiguous()   # rows (0.875, 0.125) / (0.125, 0.875)
    opts = ops.soft_loss_opts(**SOFT)
    calls["soft"] = (nat.lib.ww_ce_loss_soft_f32, (ops._ptr(z), ops._ptr(t), n, C.byref(opts), ops._ptr(d), ops._ptr(loss), ops._ptr(stats), stream), opts)
    us = {name: [] for name in calls}
    for w in range(windows + 1):                                            # window 0 warms up
        for name, (fn, args, _) in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn(*args)
            b.record()
            torch.cuda.synchronize()
            if w:
                us[name].append(1e3 * a.elapsed_time(b) / launches)
    s = ops.read_loss_stats(stats)
    assert s["batches"] == len(calls) * launches * (windows + 1) and s["bad_labels"] == 0, s
    row = {"n": n, "launches_per_window": launches, "windows": windows}
    for name, v in us.items():
        row[name] = {"us_per_call_median": statistics.median(v), "us_per_call_min": min(v), "us_per_call_max": max(v)}
    for name in ("weighted_smoothed", "focal", "soft"):
        row[f"{name}_over_plain"] = row[name]["us_per_call_median"] / row["plain"]["us_per_call_median"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the result JSON here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss.py measures on the MI355X: no GPU is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"device": nat.device_info(), "kernel": [measure(n, a.launches, a.windows, dev) for n in (16, 4096)]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
