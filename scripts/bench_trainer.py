#!/usr/bin/env python3
"""ms per training step: WakewordTrainer.step against the hand-written loop body it replaces (`run_epoch` of examples/train_from_files.py,
restated below: zero_grad, model(data), CrossEntropyLoss, clip_grad_norm_, backward, torch's Adam, loss.item(), the accuracy count and its
.item()), both models, B = 16 and B = 4096, T = 32.  Both versions run in this one process on their own copy of the model, alternating,
after a warm-up of every shape, in windows of at least `--steps` steps and `--window-ms` that end in a synchronise; each figure is the median over `--windows`
windows with their spread (min .. max).  Writes profiles/trainer_bench.json.

    PYTHONPATH=. python scripts/bench_trainer.py [--steps 20] [--windows 7] [--window-ms 300] [--out profiles/trainer_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import wakeword_jupyterlab_amd as pkg  # noqa: E402


def hand_step(model, criterion, optimizer, data, target, acc):
    """The loop body of run_epoch (examples/train_from_files.py), train branch."""
    target = target.squeeze()
    optimizer.zero_grad()
    output = model(data)
    loss = criterion(output, target)
    torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
    loss.backward()
    optimizer.step()
    acc[0] += loss.item()
    acc[1] += target.size(0)
    acc[2] += (torch.max(output.data, 1)[1] == target).sum().item()


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "trainer_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []
    for name, cls in (("SimpleWakewordModel", pkg.SimpleWakewordModel), ("WakewordModel", pkg.WakewordModel)):
        for B in (16, 4096):
            torch.manual_seed(0)
            data = -40.0 + 20.0 * torch.randn(B, 1, 80, 32, device=dev)
            target = torch.randint(0, 2, (B, 1), device=dev)
            m_hand, m_tr = cls().to(dev).train(), cls().to(dev).train()
            m_tr.load_state_dict(m_hand.state_dict())
            criterion = nn.CrossEntropyLoss().to(dev)
            optimizer = torch.optim.Adam(m_hand.parameters(), lr=1e-4, weight_decay=1e-5)
            trainer = pkg.WakewordTrainer(m_tr, dev)
            acc = [0.0, 0, 0]
            hand = lambda: hand_step(m_hand, criterion, optimizer, data, target, acc)      # noqa: E731
            fused = lambda: trainer.step(data, target)                                      # noqa: E731
            for fn in (hand, fused):
                window(fn, a.warmup)
            # a window lasts at least --window-ms of the slower version: shorter ones time the clock and the scheduler
            steps = max(a.steps, int(a.window_ms / max(window(hand, a.warmup), window(fused, a.warmup))) + 1)
            t_hand, t_fused = [], []
            for _ in range(a.windows):                                                      # alternating windows
                t_hand.append(window(hand, steps))
                t_fused.append(window(fused, steps))
            stats = pkg.ops.read_loss_stats(trainer.train_stats)                            # what the hand loop waited for twice per batch
            row = {"model": name, "batch": B, "frames": 32, "steps_per_window": steps, "windows": a.windows,
                   "hand_loop_ms": statistics.median(t_hand), "hand_loop_ms_min_max": [min(t_hand), max(t_hand)],
                   "trainer_ms": statistics.median(t_fused), "trainer_ms_min_max": [min(t_fused), max(t_fused)],
                   "ratio_hand_over_trainer": statistics.median(t_hand) / statistics.median(t_fused),
                   "trainer_batches_counted": stats["batches"], "train_math": pkg.ops.get_train_math()}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del trainer, optimizer, m_hand, m_tr
            torch.cuda.empty_cache()
    out = {"device": pkg._native.device_info(), "torch": torch.__version__, "what": "ms per training step, median over alternating windows "
           "that end in a synchronise; hand loop = run_epoch's train branch of examples/train_from_files.py", "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
