#!/usr/bin/env python3
"""ms per training step with an averaged copy of the weights: `WakewordTrainer.step` with no average, with a
fused average (the Adam launch writes it: ww_adam_avg_step_f32) and with a stand-alone `average.update()` after every step (one more
launch: ww_weight_average_f32), both models, B = 16 and B = 4096, T = 32.  The conventions of scripts/bench_trainer.py: one process, each
variant on its own copy of the model, every shape warmed up, the variants alternating in windows of at least `--steps` steps and
`--window-ms` that end in a synchronise, median and min .. max over `--windows` windows.  Writes profiles/average_bench.json.

    PYTHONPATH=. python scripts/bench_average.py [--trainer-rerun FILE] [--out profiles/average_bench.json]

`--trainer-rerun FILE`: a scripts/bench_trainer.py result of the same session; its `trainer_ms` rows and the committed
profiles/trainer_bench.json rows are set beside the no-average step.

Kernel times are taken in runs of their own (tracing slows the host):

    rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python scripts/bench_average.py --kernels simple
    python scripts/bench_average.py --merge-stats simple=DIR_SIMPLE full=DIR_FULL --out profiles/average_bench.json

`--kernels MODEL` runs 200 plain and 200 averaged steps at B = 16 and nothing else; `--merge-stats` reads adam_kernel's and
adam_avg_kernel's rows of the two runs' kernel_stats.csv into the JSON with the bytes each kernel moves (28 and 36 per element) over
its average time."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import wakeword_jupyterlab_amd as pkg  # noqa: E402

MODELS = {"simple": ("SimpleWakewordModel", pkg.SimpleWakewordModel), "full": ("WakewordModel", pkg.WakewordModel)}
VARIANTS = ("none", "fused", "stand_alone")


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def make(cls, dev, variant, state):
    model = cls().to(dev).train()
    model.load_state_dict(state)
    wa = pkg.WeightAverage(model) if variant != "none" else None
    trainer = pkg.WakewordTrainer(model, dev, average=wa if variant == "fused" else None)
    if variant == "stand_alone":
        return lambda data, target: (trainer.step(data, target), wa.update())
    return trainer.step


def overlap(a, b):
    return a[0] <= b[1] and b[0] <= a[1]


def steps_bench(a):
    dev = torch.device("cuda", 0)
    rows = []
    for name, cls in MODELS.values():
        for B in (16, 4096):
            torch.manual_seed(0)
            data = -40.0 + 20.0 * torch.randn(B, 1, 80, 32, device=dev)
            target = torch.randint(0, 2, (B, 1), device=dev)
            state = cls().state_dict()
            fns = {v: (lambda f: (lambda: f(data, target)))(make(cls, dev, v, state)) for v in VARIANTS}
            for fn in fns.values():
                window(fn, a.warmup)
            steps = max(a.steps, int(a.window_ms / max(window(fn, a.warmup) for fn in fns.values())) + 1)
            t = {v: [] for v in VARIANTS}
            for _ in range(a.windows):                                                      # alternating windows
                for v in VARIANTS:
                    t[v].append(window(fns[v], steps))
            row = {"model": name, "batch": B, "frames": 32, "steps_per_window": steps, "windows": a.windows, "train_math": pkg.ops.get_train_math()}
            for v in VARIANTS:
                row[f"{v}_ms"] = statistics.median(t[v])
                row[f"{v}_ms_min_max"] = [min(t[v]), max(t[v])]
            for v in VARIANTS[1:]:                          # per round of windows, so a drift of the machine cancels
                r = [x / y for x, y in zip(t[v], t["none"])]
                row[f"{v}_over_none"] = statistics.median(r)
                row[f"{v}_over_none_min_max"] = [min(r), max(r)]
            row["fused_and_stand_alone_ranges_overlap"] = overlap(row["fused_ms_min_max"], row["stand_alone_ms_min_max"])
            row["fused_and_none_ranges_overlap"] = overlap(row["fused_ms_min_max"], row["none_ms_min_max"])
            rows.append(row)
            print(json.dumps(row), flush=True)
            del fns
            torch.cuda.empty_cache()
    return rows


def compare_with_trainer_bench(rows, rerun_path):
    """The no-average step beside scripts/bench_trainer.py's `trainer_ms`: the committed record and, if given, a re-run of this session."""
    out = []
    sources = {"committed": os.path.join(ROOT, "profiles", "trainer_bench.json")}
    if rerun_path:
        sources["rerun_this_session"] = rerun_path
    for tag, path in sources.items():
        if not os.path.exists(path):
            continue
        for r in json.load(open(path))["rows"]:
            mine = next(x for x in rows if x["model"] == r["model"] and x["batch"] == r["batch"])
            out.append({"source": tag, "model": r["model"], "batch": r["batch"], "trainer_ms": r["trainer_ms"],
                        "trainer_ms_min_max": r["trainer_ms_min_max"], "none_ms": mine["none_ms"], "none_ms_min_max": mine["none_ms_min_max"],
                        "none_over_trainer": mine["none_ms"] / r["trainer_ms"],
                        "ranges_overlap": overlap(mine["none_ms_min_max"], r["trainer_ms_min_max"])})
    return out


def kernels_run(which):
    dev = torch.device("cuda", 0)
    _, cls = MODELS[which]
    data = -40.0 + 20.0 * torch.randn(16, 1, 80, 32, device=dev)
    target = torch.randint(0, 2, (16, 1), device=dev)
    state = cls().state_dict()
    for variant in ("none", "fused"):
        fn = make(cls, dev, variant, state)
        for _ in range(200):
            fn(data, target)
        torch.cuda.synchronize()


def merge_stats(pairs, out_path):
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    rows = []
    for pair in pairs:
        which, d = pair.split("=", 1)
        name, cls = MODELS[which]
        elements = sum(p.numel() for p in cls().parameters())
        found = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
        if not found:
            raise SystemExit(f"no *kernel_stats.csv under {d}")
        for r in csv.DictReader(open(found[0])):
            kernel = r["Name"]
            per = 36 if "adam_avg_kernel" in kernel else 28 if "adam_kernel" in kernel else None
            if per is None:
                continue
            avg_ns = float(r["AverageNs"])
            rows.append({"model": name, "kernel": "adam_avg_kernel" if per == 36 else "adam_kernel", "calls": int(r["Calls"]),
                         "average_us": avg_ns / 1e3, "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3,
                         "elements": elements, "bytes_per_element": per, "bytes": per * elements, "gb_per_s": per * elements / avg_ns})
    doc["adam_kernels"] = {"what": "rocprofv3 --kernel-trace --stats, a run of its own per model: 200 steps per kernel at B = 16 (the Adam "
                                   "launch does not depend on B), the first step of the averaged kernel runs the copy rule (32 bytes per "
                                   "element); bytes = bytes_per_element x the model's parameter count, gb_per_s = bytes / average time",
                           "rows": rows}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in rows:
        print(json.dumps(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--trainer-rerun", default=None)
    ap.add_argument("--kernels", choices=sorted(MODELS), default=None)
    ap.add_argument("--merge-stats", nargs="+", default=None, metavar="MODEL=DIR")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "average_bench.json"))
    a = ap.parse_args()
    if a.merge_stats:
        return merge_stats(a.merge_stats, a.out)
    if a.kernels:
        return kernels_run(a.kernels)
    rows = steps_bench(a)
    out = {"device": pkg._native.device_info(), "torch": torch.__version__,
           "what": "ms per training step, median over alternating windows that end in a synchronise: none = WakewordTrainer.step, fused = the "
                   "same with average=WeightAverage(model) (written by the Adam launch), stand_alone = the plain step followed by "
                   "WeightAverage.update() (one more launch); *_over_none = the median and min .. max of the per-round ratios",
           "rows": rows, "against_trainer_bench": compare_with_trainer_bench(rows, a.trainer_rerun)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
