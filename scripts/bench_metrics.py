#!/usr/bin/env python3
"""Clip evaluation as device counters: the update kernel alone, and one evaluation pass through
`inference.evaluate` (the reference's loop: two device-to-host waits and a per-clip host list per batch) against
`inference.evaluate_report` (one launch per batch, one copy at the end).

    PYTHONPATH=. python scripts/bench_metrics.py [--launches 200] [--windows 9] [--clips 32768] [--passes 7] [--out profiles/metrics_bench.json]

kernel: ww_clip_metrics_update_f32 at n = 16, 256 and 4096 with three operating points, the C entry point itself with its arguments
prepared once.  One device-event pair around `--launches` back-to-back calls per window, `--windows` windows after a warm-up window;
median and range of the windows, in microseconds per call.  Back-to-back calls on one stream serialise on the record, so this is the
time from one call's start to the next one's, launch overhead included -- what a batch of an evaluation loop pays.
pass: `--clips` synthetic one-second clips in a ClipBank (64 distinct ones, tiled), labels alternating, SimpleWakewordModel with seeded
weights; one pass = the bank's loader at batch 4096 and at batch 16, through both functions, alternating pass for pass after a warm-up
pass each, wall time around a pass that ends in a device synchronise.  Both passes pay the same loader and the same forward; the
confusion matrices of the two are compared before anything is timed."""
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
from wakeword_jupyterlab_amd import inference, ops  # noqa: E402

THRESHOLDS = (0.5, 0.8, 0.999)


def measure_kernel(launches, windows, dev):
    res = []
    g = torch.Generator().manual_seed(0)
    for n in (16, 256, 4096):
        z = (torch.randn(n, 2, generator=g) * 6.0).to(dev)
        y = (torch.rand(n, generator=g) < 0.1).to(torch.int64).to(dev)
        state = ops.new_clip_metrics(dev, THRESHOLDS)
        args = (ops._ptr(z), ops._ptr(y), n, ops._ptr(state.buffer), ops._stream())
        us = []
        for w in range(windows + 1):                                        # window 0 warms up
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                nat.lib.ww_clip_metrics_update_f32(*args)
            b.record()
            torch.cuda.synchronize()
            if w:
                us.append(1e3 * a.elapsed_time(b) / launches)
        r = ops.read_clip_metrics(state)
        assert r.clips_seen == n * launches * (windows + 1) and r.batches == launches * (windows + 1)
        res.append({"n": n, "thresholds": len(THRESHOLDS), "launches_per_window": launches, "windows": windows,
                    "us_per_call_median": statistics.median(us), "us_per_call_min": min(us), "us_per_call_max": max(us)})
    return res


def measure_pass(clips, passes, dev):
    proc = pkg.AudioProcessor(device=dev)
    pcm = torch.from_numpy(pkg.synth.make_clips_tiled(0, clips, unique=64, n=16000)).to(dev)
    bank = pkg.ClipBank(proc)
    bank.add_pcm(pcm[0::2], 0)
    bank.add_pcm(pcm[1::2], 1)
    del pcm
    sd = pkg.synth.make_state_dict("simple", seed=1234)
    model = pkg.SimpleWakewordModel()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(dev).eval()
    out = {"clips": clips, "passes": passes, "model": "simple", "thresholds": len(THRESHOLDS)}
    for batch in (4096, 16):
        loader = bank.loader(batch, shuffle=False)

        def run_evaluate():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            preds, labels = inference.evaluate(model, loader, dev)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, (preds, labels)

        def run_report():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            report = inference.evaluate_report(model, loader, dev, thresholds=THRESHOLDS)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, report
        _, (preds, labels) = run_evaluate()                                 # warm-up passes, and the two must agree
        _, report = run_report()
        conf = np.zeros((2, 2), np.int64)
        np.add.at(conf, (np.asarray(labels, np.int64), np.asarray(preds, np.int64)), 1)
        assert np.array_equal(conf, report.confusion) and report.total == clips, (conf, report.confusion)
        wall = {"evaluate": [], "evaluate_report": []}
        for _ in range(passes):                                             # alternating pass for pass
            wall["evaluate"].append(run_evaluate()[0])
            wall["evaluate_report"].append(run_report()[0])
        row = {"batch": batch, "batches_per_pass": len(loader)}
        for k, v in wall.items():
            row[k] = {"ms_per_pass_median": 1e3 * statistics.median(v), "ms_per_pass_min": 1e3 * min(v), "ms_per_pass_max": 1e3 * max(v),
                      "ms_per_pass_all": [1e3 * t for t in v]}
        row["report_over_evaluate"] = row["evaluate_report"]["ms_per_pass_median"] / row["evaluate"]["ms_per_pass_median"]
        row["ranges_overlap"] = not (row["evaluate_report"]["ms_per_pass_max"] < row["evaluate"]["ms_per_pass_min"]
                                     or row["evaluate"]["ms_per_pass_max"] < row["evaluate_report"]["ms_per_pass_min"])
        out[f"batch_{batch}"] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--clips", type=int, default=32768)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the result JSON here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py measures on the MI355X: no GPU is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"device": nat.device_info(), "kernel": measure_kernel(a.launches, a.windows, dev), "pass": measure_pass(a.clips, a.passes, dev)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
