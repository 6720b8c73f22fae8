#!/usr/bin/env python3
"""What quantisation-aware training costs, both models.  Writes profiles/qat_bench.json.

  launch     ms per quantisation of all weight matrices on prepared tables: ww_quant_weights_clip_f32 under the searched clip indices beside
             ww_quant_weights_f32 on the same tensors (the same bytes plus one byte per row)
  search     ms per ww_quant_clip_search_f32 over the same tensors with one scale per row and with one scale per tensor (one workgroup per
             matrix: slow, and not on a per-step path)
  ste        ms per ww_quant_ste_f32 over the weight matrices' gradients beside a device-to-device copy of the same float32 bytes
  step       ms per WakewordTrainer.step at B = 16 and B = 4096 (T = 32): this tree's plain step, qat=True with clip="max" (one more
             launch) and with clip="mse" (two more), 4 bits, in one process -- the parent commit's build was not run beside it
  deviation  SQNR of the weights and the largest difference in a logit between WeightQuant.model and the float32 model at 8, 6 and 4
             bits under clip="max" and clip="mse", on the seed-1234 synthetic weights and the synthetic clips of scripts/bench_quant.py:
             no accuracy figure on real speech is measured here

The conventions of scripts/bench_quant.py: one process, everything warmed up, the variants alternating in windows that end in a
synchronise, median and min .. max over `--windows` windows.

    PYTHONPATH=. python scripts/bench_qat.py [--out profiles/qat_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402

import wakeword_jupyterlab_amd as pkg  # noqa: E402
from bench_quant import MODELS, golden_model, window  # noqa: E402
from wakeword_jupyterlab_amd import ops  # noqa: E402


def alternate(a, fns, steps=None):
    """{variant: [ms per call per window]} over alternating windows; `steps` calls per window, or enough to fill --window-ms."""
    for fn in fns.values():
        window(fn, 2 if steps else a.warmup)
    if steps is None:
        steps = max(a.steps, int(a.window_ms / max(window(fn, a.warmup) for fn in fns.values())) + 1)
    t = {v: [] for v in fns}
    for _ in range(a.windows):
        for v, fn in fns.items():
            t[v].append(window(fn, steps))
    return t, steps


def summary(t, base=None):
    row = {}
    for v, xs in t.items():
        row[f"{v}_ms"] = statistics.median(xs)
        row[f"{v}_ms_min_max"] = [min(xs), max(xs)]
        if base is not None and v != base:                   # per round of windows, so a drift of the machine cancels
            r = [x / y for x, y in zip(xs, t[base])]
            row[f"{v}_over_{base}"] = statistics.median(r)
            row[f"{v}_over_{base}_min_max"] = [min(r), max(r)]
    return row


def kernels(a, arch, dev, bits=4):
    model = golden_model(arch, dev)
    weights = [p.detach() for p in model.parameters() if p.dim() >= 2]
    elements = sum(w.numel() for w in weights)
    row = {"model": MODELS[arch][0], "bits": bits, "tensors": len(weights), "rows": sum(w.shape[0] for w in weights), "elements": elements,
           "float32_bytes": 4 * elements, "windows": a.windows}
    # the clipped launch beside the plain one
    found = ops.quant_clip_search(weights, bits=bits, cand_err=False)
    clips = [f[0] for f in found]
    plain = ops.quantize_weights(weights, bits=bits)
    clipped = ops.quantize_weights_clip(weights, clips, bits=bits)
    t_plain = ops.quant_table(weights, *([o[j] for o in plain] for j in (1, 0, 2, 3, 4)))
    t_clip = ops.quant_clip_table(weights, [o[1] for o in clipped], clips, *([o[j] for o in clipped] for j in (0, 2, 3, 4, 5)))
    t, steps = alternate(a, {"plain": lambda: ops.quantize_weights_launch(t_plain, dev, bits),
                             "clipped": lambda: ops.quantize_weights_clip_launch(t_clip, dev, bits)})
    row.update(summary(t, "plain"), launch_calls_per_window=steps)
    # the straight-through launch beside a copy of the same bytes
    grads = [torch.randn_like(w) for w in weights]
    src, dst = torch.randn(elements, device=dev), torch.empty(elements, device=dev)
    t_ste = ops.quant_ste_table(weights, [o[1] for o in clipped], grads)
    t, steps = alternate(a, {"copy": lambda: dst.copy_(src), "ste": lambda: ops.quant_ste_launch(t_ste, dev, bits)})
    row.update(summary(t, "copy"), ste_calls_per_window=steps, saturated_elements=int(sum(int(o[5].sum()) for o in clipped)))
    # the search, per row and per tensor
    for name, per_channel, steps in (("search_rows", True, None), ("search_tensor", False, 3)):
        out = ops.quant_clip_search(weights, bits=bits, per_channel=per_channel, cand_err=False)
        tab = ops.quant_clip_table(weights, [o[1] for o in out], [o[0] for o in out], per_channel=per_channel)
        t, n = alternate(a, {name: lambda tab=tab: ops.quant_clip_search_launch(tab, dev, bits)}, steps)
        row.update(summary(t), **{f"{name}_calls_per_window": n})
    return row


def steps(a, arch, dev, B, bits=4):
    x = (-40.0 + 20.0 * torch.randn(B, 1, 80, 32, device=dev))
    y = torch.randint(0, 2, (B,), device=dev)
    fns = {}
    for name, clip in (("plain", None), ("qat_max", "max"), ("qat_mse", "mse")):
        model = golden_model(arch, dev).train()
        wq = None if clip is None else pkg.WeightQuant(model, bits=bits, clip=clip)
        trainer = pkg.WakewordTrainer(model, dev, quant=wq, qat=wq is not None, qat_calibrate=None)
        fns[name] = lambda trainer=trainer: trainer.step(x, y)
    t, n = alternate(a, fns)
    return dict({"model": MODELS[arch][0], "batch": B, "frames": 32, "bits": bits, "calls_per_window": n, "windows": a.windows}, **summary(t, "plain"))


def deviation(arch, dev, clips):
    model = golden_model(arch, dev)
    pcm = torch.from_numpy(pkg.synth.make_clips(0, clips)).to(dev)
    rows = []
    with torch.no_grad():
        z = model.forward_pcm(pcm).double()
        for bits in (8, 6, 4):
            for clip in ("max", "mse"):
                wq = pkg.WeightQuant(model, bits=bits, clip=clip)
                rep = wq.report().totals
                rows.append({"model": MODELS[arch][0], "bits": bits, "clip": clip, "clips": clips, "weights_sqnr_db": rep["sqnr_db"],
                             "weights_max_error": rep["max_error"], "max_logit_deviation": float((wq.model.forward_pcm(pcm).double() - z).abs().max()),
                             "saturated": rep.get("saturated", 0), "clip_fraction_min": rep.get("clip_min", 1.0),
                             "clip_fraction_mean": rep.get("clip_mean", 1.0)})
                print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 4096])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qat_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1234)
    out = {"device": pkg._native.device_info(), "torch": torch.__version__,
           "what": "ms per call, median and min .. max over alternating windows that end in a synchronise; *_over_* = the median and "
                   "min .. max of the per-round ratios.  kernels: plain = ww_quant_weights_f32, clipped = ww_quant_weights_clip_f32 under "
                   "the searched indices (all outputs written), ste = ww_quant_ste_f32 beside copy = one device-to-device copy of the "
                   "same float32 bytes, search_rows / search_tensor = ww_quant_clip_search_f32 with one scale per row / per tensor.  "
                   "steps: WakewordTrainer.step of this tree without a quantiser and with qat=True, in one process; the parent "
                   "commit's build was not measured beside it.  deviation: synthetic weights (seed 1234) and synthetic clips; not an "
                   "accuracy figure: no real speech was used",
           "kernels": [], "steps": [], "deviation": []}
    for arch in MODELS:
        out["kernels"].append(kernels(a, arch, dev))
        print(json.dumps(out["kernels"][-1]), flush=True)
    for arch in MODELS:
        for B in a.batches:
            out["steps"].append(steps(a, arch, dev, B))
            print(json.dumps(out["steps"][-1]), flush=True)
    for arch in MODELS:
        out["deviation"] += deviation(arch, dev, a.clips)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
