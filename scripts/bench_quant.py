#!/usr/bin/env python3
"""What post-training weight quantisation costs, both models.  Writes profiles/quant_bench.json.

  launch     ms per quantisation of all weight matrices on prepared tables (ww_quant_weights_f32: one launch for the 7 / 8 tensors), with one
             scale per row and with one scale per tensor, beside a device-to-device copy of the same float32 bytes -- the project's
             usual yardstick for a memory-bound kernel, not a pass mark: the kernel is not on a per-step path
  update     WeightQuant.update() end to end: the launch, the version counters, the float32 copies of the biases
  deviation  the largest difference in a logit and in the margin z1 - z0 between WeightQuant.model and the float32 model at 8, 6 and
             4 bits, on the weights of tests/golden/model_*_seed1234.npz (synth.make_state_dict(arch, seed=1234)) and the seeded
             synth.make_clips -- synthetic weights on synthetic audio: no accuracy figure on real speech is measured here

The conventions of scripts/bench_average.py: one process, everything warmed up, the variants alternating in windows of at least `--steps`
calls and `--window-ms` that end in a synchronise, median and min .. max over `--windows` windows.

    PYTHONPATH=. python scripts/bench_quant.py [--out profiles/quant_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import wakeword_jupyterlab_amd as pkg  # noqa: E402
from wakeword_jupyterlab_amd import ops  # noqa: E402

MODELS = {"simple": ("SimpleWakewordModel", pkg.SimpleWakewordModel), "full": ("WakewordModel", pkg.WakewordModel)}
VARIANTS = ("copy", "launch_rows", "launch_tensor", "update")


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def golden_model(arch, dev):
    model = MODELS[arch][1]()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in pkg.synth.make_state_dict(arch, seed=1234).items()})
    return model.to(dev).eval()


def launcher(weights, dev, per_channel):
    outs = ops.quantize_weights(weights, bits=8, per_channel=per_channel)
    q, scale, deq, err, bad = ([o[j] for o in outs] for j in range(5))
    table = ops.quant_table(weights, scale, q, deq, err, bad, per_channel=per_channel)
    return lambda: ops.quantize_weights_launch(table, dev, 8)


def timing(a, arch, dev):
    model = golden_model(arch, dev)
    weights = [p.detach() for p in model.parameters() if p.dim() >= 2]
    elements = sum(w.numel() for w in weights)
    src, dst = torch.randn(elements, device=dev), torch.empty(elements, device=dev)
    wq = pkg.WeightQuant(model)
    fns = {"copy": lambda: dst.copy_(src), "launch_rows": launcher(weights, dev, True), "launch_tensor": launcher(weights, dev, False),
           "update": wq.update}
    for fn in fns.values():
        window(fn, a.warmup)
    steps = max(a.steps, int(a.window_ms / max(window(fn, a.warmup) for fn in fns.values())) + 1)
    t = {v: [] for v in VARIANTS}
    for _ in range(a.windows):                                                              # alternating windows
        for v in VARIANTS:
            t[v].append(window(fns[v], steps))
    row = {"model": MODELS[arch][0], "tensors": len(weights), "rows": sum(w.shape[0] for w in weights), "elements": elements,
           "float32_bytes": 4 * elements, "calls_per_window": steps, "windows": a.windows}
    for v in VARIANTS:
        row[f"{v}_ms"] = statistics.median(t[v])
        row[f"{v}_ms_min_max"] = [min(t[v]), max(t[v])]
    for v in VARIANTS[1:]:                                  # per round of windows, so a drift of the machine cancels
        r = [x / y for x, y in zip(t[v], t["copy"])]
        row[f"{v}_over_copy"] = statistics.median(r)
        row[f"{v}_over_copy_min_max"] = [min(r), max(r)]
    return row


def deviation(arch, dev, clips):
    model = golden_model(arch, dev)
    pcm = torch.from_numpy(pkg.synth.make_clips(0, clips)).to(dev)
    rows = []
    with torch.no_grad():
        z = model.forward_pcm(pcm).double()
        margin = z[:, 1] - z[:, 0]
        for per_channel in (True, False):
            for bits in (8, 6, 4):
                wq = pkg.WeightQuant(model, bits=bits, per_channel=per_channel)
                zq = wq.model.forward_pcm(pcm).double()
                mq = zq[:, 1] - zq[:, 0]
                rep = wq.report().totals
                rows.append({"model": MODELS[arch][0], "bits": bits, "per_channel": per_channel, "clips": clips,
                             "max_logit_deviation": float((zq - z).abs().max()), "max_margin_deviation": float((mq - margin).abs().max()),
                             "float32_margin_min_max": [float(margin.min()), float(margin.max())],
                             "decisions_changed": int(((mq > 0) != (margin > 0)).sum()), "weights_sqnr_db": rep["sqnr_db"],
                             "weights_max_error": rep["max_error"], "fp32_bytes": rep["fp32_bytes"], "int8_bytes": rep["int8_bytes"],
                             "float_bytes": rep["float_bytes"]})
                print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quant_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    timings = []
    for arch in MODELS:
        timings.append(timing(a, arch, dev))
        print(json.dumps(timings[-1]), flush=True)
    deviations = [r for arch in MODELS for r in deviation(arch, dev, a.clips)]
    out = {"device": pkg._native.device_info(), "torch": torch.__version__,
           "what": "timing: ms per call, median over alternating windows that end in a synchronise -- copy = one device-to-device copy of "
                   "the weight matrices' float32 bytes, launch_rows / launch_tensor = ww_quant_weights_f32 over all of them on a prepared "
                   "table with one scale per row / per tensor (q, scale, deq, err and bad written), update = WeightQuant.update(); "
                   "*_over_copy = the median and min .. max of the per-round ratios.  deviation: WeightQuant.model against the float32 "
                   "model on synthetic weights (seed 1234) and synthetic clips (synth.make_clips(0, clips)), logits through forward_pcm; "
                   "not an accuracy figure: no real speech was used",
           "timing": timings, "deviation": deviations}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
