#!/usr/bin/env python3
"""What knowledge distillation costs on the MI355X, two measurements in one process:

  kernel   ww_distill_loss_f32 (integer labels with options, alpha 0.5, T 2) beside ww_ce_loss_ex_f32 on the same logits and labels at
           n = 16 and n = 4096: device events around `--launches` back-to-back calls per window, the two alternating window by window
           after a warm-up window each; microseconds per call and the ratio, beside the ratio of the bytes each reads per clip (logits,
           teacher logits and labels: 24 against 16; the pass in front reads teacher logits and labels once more)
  step     WakewordTrainer.step with a teacher of the OTHER model class, for both student classes at B = 16 and B = 4096, T = 32, beside
             hand    the best the public pieces allowed before: teacher(x) under no_grad, the train-mode forward through autograd
                     (ops.train_forward), a loss composed in torch -- (1 - alpha) F.cross_entropy + alpha T^2 F.kl_div(batchmean) --,
                     loss.backward() and FusedAdam
             plain   the same trainer class without a teacher
             teacher the teacher's eval forward alone (model(x) under no_grad): the floor of what a teacher can add to the plain step
           four callables on their own copies of the models, alternating windows that end in a synchronise

Every figure is the median over the windows with their spread (min .. max).  Writes profiles/distill_bench.json.

    PYTHONPATH=. python scripts/bench_distill.py [--launches 200] [--windows 7] [--out profiles/distill_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import wakeword_jupyterlab_amd as pkg  # noqa: E402
from wakeword_jupyterlab_amd import _native as nat  # noqa: E402
from wakeword_jupyterlab_amd import ops  # noqa: E402

ALPHA, TEMPERATURE = 0.5, 2.0


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def bench_kernel(dev, launches, windows):
    rows = []
    for n in (16, 4096):
        g = torch.Generator().manual_seed(n)
        z, zt = (4.0 * torch.randn(n, 2, generator=g)).to(dev), (4.0 * torch.randn(n, 2, generator=g)).to(dev)
        y = torch.randint(0, 2, (n,), generator=g).to(dev)
        d, loss, stats, dstats = torch.empty_like(z), torch.empty((), device=dev), ops.new_loss_stats(dev), ops.new_distill_stats(dev)
        opts = ops.loss_opts(weight=(0.25, 4.0), label_smoothing=0.125)
        ops.ce_loss_into(z, y, d, loss, stats, opts=opts)                        # the checked calls once; then the C entries with prepared arguments
        ops.distill_loss_into(z, zt, y, d, loss, stats, dstats, alpha=ALPHA, temperature=TEMPERATURE, opts=opts)
        stream = ops._stream()
        ce_args = (ops._ptr(z), ops._ptr(y), n, C.byref(opts), ops._ptr(d), ops._ptr(loss), ops._ptr(stats), stream)
        kd_args = (ops._ptr(z), ops._ptr(zt), ops._ptr(y), nat.TARGET_LABELS, n, C.byref(opts), ALPHA, TEMPERATURE, ops._ptr(d), ops._ptr(loss),
                   ops._ptr(stats), ops._ptr(dstats), stream)
        variants = {"ce_loss_ex": lambda a=ce_args: nat.check(nat.lib.ww_ce_loss_ex_f32(*a)),
                    "distill_loss": lambda a=kd_args: nat.check(nat.lib.ww_distill_loss_f32(*a))}
        us = {name: [] for name in variants}
        for w in range(windows + 1):                                            # window 0 warms up both
            for name, fn in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(launches):
                    fn()
                b.record()
                torch.cuda.synchronize()
                if w:
                    us[name].append(1e3 * a.elapsed_time(b) / launches)
        row = {"n": n, "launches_per_window": launches, "windows": windows, "ce_loss_ex_us": spread(us["ce_loss_ex"]),
               "distill_loss_us": spread(us["distill_loss"]),
               "distill_over_ce_time": statistics.median(us["distill_loss"]) / statistics.median(us["ce_loss_ex"]),
               "distill_over_ce_bytes_read_per_clip": 24 / 16, "with_the_pass_in_front": (24 + 16) / (16 + 8)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def bench_step(dev, windows, min_steps=10, window_ms=500.0, warmup=3):
    classes = {"SimpleWakewordModel": pkg.SimpleWakewordModel, "WakewordModel": pkg.WakewordModel}
    rows = []
    for student, teacher in (("SimpleWakewordModel", "WakewordModel"), ("WakewordModel", "SimpleWakewordModel")):
        for B in (16, 4096):
            torch.manual_seed(0)
            data = -40.0 + 20.0 * torch.randn(B, 1, 80, 32, device=dev)
            y = torch.randint(0, 2, (B,), device=dev)
            t = classes[teacher]().to(dev).eval()
            m_fused, m_hand, m_plain = (classes[student]().to(dev).train() for _ in range(3))
            for m in (m_hand, m_plain):
                m.load_state_dict(m_fused.state_dict())
            fused = pkg.WakewordTrainer(m_fused, dev, teacher=t, distill_alpha=ALPHA, distill_temperature=TEMPERATURE)
            plain = pkg.WakewordTrainer(m_plain, dev)
            opt = pkg.FusedAdam(m_hand.parameters(), lr=pkg.TrainingConfig.LEARNING_RATE, weight_decay=1e-5)

            def f_hand():
                with torch.no_grad():
                    zt = t(data)
                z = m_hand(data)
                kd = F.kl_div(F.log_softmax(z / TEMPERATURE, dim=1), F.softmax(zt / TEMPERATURE, dim=1), reduction="batchmean")
                loss = (1.0 - ALPHA) * F.cross_entropy(z, y) + ALPHA * TEMPERATURE * TEMPERATURE * kd
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()

            def f_teacher():
                with torch.no_grad():
                    t(data)
            fns = {"fused": lambda: fused.step(data, y), "hand": f_hand, "plain": lambda: plain.step(data, y), "teacher": f_teacher}
            for fn in fns.values():
                window(fn, warmup)
            steps = max(min_steps, int(window_ms / max(window(fn, warmup) for fn in fns.values())) + 1)
            ms = {name: [] for name in fns}
            for _ in range(windows):                                                        # alternating windows
                for name, fn in fns.items():
                    ms[name].append(window(fn, steps))
            med = {name: statistics.median(v) for name, v in ms.items()}
            row = {"student": student, "teacher": teacher, "batch": B, "frames": 32, "steps_per_window": steps, "windows": windows,
                   "fused_ms": spread(ms["fused"]), "hand_loop_ms": spread(ms["hand"]), "plain_step_ms": spread(ms["plain"]),
                   "teacher_eval_forward_ms": spread(ms["teacher"]), "fused_over_hand": med["fused"] / med["hand"],
                   "fused_minus_plain_ms": med["fused"] - med["plain"],
                   "fused_range_at_or_below_hand_range": max(ms["fused"]) <= max(ms["hand"]) and min(ms["fused"]) <= min(ms["hand"]),
                   "train_math": ops.get_train_math()}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del fused, plain, opt, m_fused, m_hand, m_plain, t
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "distill_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_distill.py measures on the MI355X: no GPU is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"device": nat.device_info(), "torch": torch.__version__, "alpha": ALPHA, "temperature": TEMPERATURE,
           "what": "median (min .. max) over alternating windows after a warm-up of every variant; kernel: device events around back-to-back "
                   "calls; step: a host clock around work that ends in a synchronise"}
    out["kernel"] = bench_kernel(dev, a.launches, a.windows)
    out["step"] = bench_step(dev, a.windows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
