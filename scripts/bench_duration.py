"""Cost of clips longer than 1 s (inference): K1 (ww_logmel_frames_f32) and K2 (ww_cnn_pool_wide_f32, column-tiled above 32 frames) per
4,096 clips at 1 s, 1.5 s and 2 s, both models, default arithmetic (auto log-mel, f16x3 convs).  The tiled conv stack runs K 32-column
tiles per clip (K = 2 / 3 at T = 47 / 63 for both models), so its predicted cost is K x the 1 s conv stack; the line reports the measured
ratio next to K.  Augmentation (KA, ww_augment_f32 at 1 s, ww_augment_n_f32 below) per 4,096 clips at 0.25 / 0.5 / 0.75 / 1 s with the
reference's plan mix (each transform with p = 0.8, AudioProcessor.draw_augment_plan), and the training data path + step at 0.5 s and 1 s:
PCM in HBM -> augment -> normalise + log-mel -> 2-conv train-mode forward + CrossEntropyLoss + backward + Adam.  One JSON line.
Alone: PYTHONPATH=. python scripts/bench_duration.py"""
import json
import random
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_ms(fn, warmup=3, steps=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def _plans(proc, batch):
    from wakeword_jupyterlab_amd import _native as nat
    arr = (nat.AugmentPlan * batch)()
    for a in arr:
        p = proc.draw_augment_plan()                              # the product's own draws (reference order, python `random`)
        a.shift, a.crop_start = p["shift"], p["crop"]
        a.pitch_rate = 2.0 ** (-p["n_steps"] / 12.0) if p["n_steps"] is not None else 0.0
        a.stretch_rate = p["rate"] or 0.0
        a.noise_sigma, a.noise_seed = p["sigma"], p["seed"]
    return arr


def _cfg(duration):
    from wakeword_jupyterlab_amd.config import AudioConfig
    return type("Cfg", (AudioConfig,), {"DURATION": duration})


def augment_legs(batch, dev):
    """clips/s of the augmentation at each clip length; the plans are drawn once per length (host draws not timed)"""
    import numpy as np
    import wakeword_jupyterlab_amd as pkg
    from wakeword_jupyterlab_amd import ops
    legs, base = {}, None
    for dur in (1.0, 0.75, 0.5, 0.25):
        n = int(16000 * dur)
        x = pkg.synth.make_clips_tiled(0, batch, unique=64, n=n)
        pcm = torch.from_numpy(x / np.abs(x).max(axis=1, keepdims=True)).float().to(dev)
        random.seed(0)
        arr = _plans(pkg.AudioProcessor(_cfg(dur)), batch)
        ms = _time_ms(lambda: ops.augment(pcm, arr), warmup=2, steps=10)
        base = base or ms
        legs[f"{dur}s"] = {"N": n, "T": 1 + n // 512, "ms": round(ms, 3), "clips_per_s": round(batch / ms * 1e3), "rate_over_1s": round(base / ms, 3)}
        del pcm
    return legs


def train_pipeline(batch, dev, dur, steps=4):
    """augment -> log-mel -> training step at one clip length, new plans every step (drawn on the host, not timed)"""
    import numpy as np
    import wakeword_jupyterlab_amd as pkg
    from wakeword_jupyterlab_amd import ops
    cfg = _cfg(dur)
    n = int(16000 * dur)
    sd = pkg.synth.make_state_dict("simple", seed=1234)
    m = pkg.SimpleWakewordModel(audio_config=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(dev).train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    crit = torch.nn.CrossEntropyLoss()
    x = pkg.synth.make_clips_tiled(0, batch, unique=64, n=n)
    pcm = torch.from_numpy(x / np.abs(x).max(axis=1, keepdims=True)).float().to(dev)
    y = torch.randint(0, 2, (batch,), device=dev)
    random.seed(0)
    proc = pkg.AudioProcessor(cfg)
    plans = [_plans(proc, batch) for _ in range(steps + 1)]

    def step(arr):
        mel = ops.logmel_frames(ops.augment(pcm, arr), n, True)
        opt.zero_grad()
        loss = crit(m(mel), y)
        loss.backward()
        opt.step()
        return loss
    step(plans[0])
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(steps):
        loss = step(plans[i + 1])
    b.record()
    torch.cuda.synchronize(dev)
    ms = a.elapsed_time(b) / steps
    return {"N": n, "T": 1 + n // 512, "ms_per_batch": round(ms, 3), "clips_per_s": round(batch / ms * 1e3), "final_loss": round(float(loss.item()), 5)}


def main(batch=4096):
    import wakeword_jupyterlab_amd as pkg
    from wakeword_jupyterlab_amd import ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"batch": batch, "logmel_math": ops.get_logmel_math(), "conv_math": ops.get_conv_math(), "legs": {}}
    for arch, n_conv in (("simple", 2), ("full", 3)):
        packed = torch.from_numpy(ops.pack_state_dict(pkg.synth.make_state_dict(arch, seed=1234))).to(dev)
        base = None
        for dur in (1.0, 1.5, 2.0):
            n = int(16000 * dur)
            pcm = torch.from_numpy(pkg.synth.make_clips_tiled(0, batch, unique=256, n=n)).to(dev)
            mel = ops.logmel_frames(pcm, n, True)
            T = mel.shape[3]
            k1 = _time_ms(lambda: ops.logmel_frames(pcm, n, True))
            k2 = _time_ms(lambda: ops.cnn_pool_wide(mel, packed, n_conv))
            tiles = 1 if T <= 32 else 1 + -(-(T - 32) // (32 - 2 * (n_conv)))
            if base is None:
                base = k2
            out["legs"][f"{arch}_{dur}s"] = {"T": T, "K1_ms": round(k1, 4), "K2_ms": round(k2, 4), "tiles": tiles,
                                             "K2_over_1s": round(k2 / base, 3), "tiling_overhead_vs_prediction": round(k2 / (base * tiles), 3)}
            del pcm, mel
    out["augment"] = augment_legs(batch, dev)
    out["train_pipeline_simple"] = {f"{dur}s": train_pipeline(batch, dev, dur) for dur in (1.0, 0.5)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
