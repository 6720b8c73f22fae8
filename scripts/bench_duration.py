"""Cost of clips longer than 1 s (inference): K1 (ww_logmel_frames_f32) and K2 (ww_cnn_pool_wide_f32, column-tiled above 32 frames) per
4,096 clips at 1 s, 1.5 s and 2 s, both models, default arithmetic (auto log-mel, f16x3 convs).  The tiled conv stack runs K 32-column
tiles per clip (K = 2 / 3 at T = 47 / 63 for both models), so its predicted cost is K x the 1 s conv stack; the line reports the measured
ratio next to K.  One JSON line.  Alone: PYTHONPATH=. python scripts/bench_duration.py"""
import json
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
    print(json.dumps(out))


if __name__ == "__main__":
    main()
