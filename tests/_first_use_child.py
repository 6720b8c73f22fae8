"""The paths of tests/test_gpu_first_use.py (not a test module itself).

`run(path)` makes one call into the library and returns the bytes it produced.  As a script (`_first_use_child.py <path>`) that call is
the process's first GPU work, so every kernel behind it is launched -- and, above 64 KiB of dynamic LDS, opted in -- for the first
time; it prints `FIRST_USE <path> <sha256 of the bytes> <ww_sync_timeouts()>`.  The test makes the same call in its own, warm process
and compares the hashes: the kernels give the same bits for any batch or grid, so no tolerance is needed.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import wakeword_jupyterlab_amd as pkg  # noqa: E402
from wakeword_jupyterlab_amd import _native as nat, ops  # noqa: E402

PATHS = ("frames_f16x3", "frames_f32", "pcm_f16x3d", "train3_f16x3", "train2_f32", "augment", "streamer")


def _model(arch, dev):
    sd = pkg.synth.make_state_dict(arch, seed=1234)
    model = pkg.SimpleWakewordModel() if arch == "simple" else pkg.WakewordModel()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.to(dev).eval()


def _forward(dev, conv_math, n_samples):
    """2 clips through the 3-conv model: 17,408 samples are 35 frames, two column tiles; 16,000 the 1 s kernels"""
    model = _model("full", dev)
    pcm = torch.from_numpy(pkg.synth.make_clips(0, 2, n_samples)).to(dev)
    packed = model.packed_weights()
    before = ops.get_conv_math()
    ops.set_conv_math(conv_math)
    try:
        if n_samples == 16000:
            logits = ops.forward_pcm(pcm, packed, 3)
        else:
            logits = ops.forward_pcm_frames(pcm, packed, 3, n_samples)
        return logits.cpu().numpy().tobytes()
    finally:
        ops.set_conv_math(before)


def _train(dev, arch, train_math):
    """one training forward and backward, B = 2, T = 32, fixed dropout seed: the logits and every gradient"""
    n_conv = 2 if arch == "simple" else 3
    sd = pkg.synth.make_state_dict(arch, seed=1234)
    params = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in sd.items()}
    x = torch.from_numpy((20.0 * pkg.synth.normal(77, 2 * 80 * 32) - 40.0).astype(np.float32).reshape(2, 1, 80, 32)).to(dev)
    dlogits = torch.from_numpy(np.array([[0.25, -0.25], [-0.5, 0.5]], dtype=np.float32)).to(dev)
    before = ops.get_train_math()
    ops.set_train_math(train_math)
    try:
        logits = ops.train_forward(x, params, n_conv, 0.5, 0.5, 1234)
        logits.backward(dlogits)
        return b"".join([logits.detach().cpu().numpy().tobytes()] + [params[k].grad.cpu().numpy().tobytes() for k in ops._train_keys(n_conv)])
    finally:
        ops.set_train_math(before)


def _augment(dev):
    """a pitch plan and a stretch plan: the vocoder and resampler kernels"""
    pcm = torch.from_numpy(pkg.synth.make_clips(0, 2)).to(dev)
    plans = [dict(shift=100, n_steps=2.0, sigma=0.01, seed=5), dict(rate=0.9, crop=100, sigma=0.01, seed=6)]
    return ops.augment(pcm, plans).cpu().numpy().tobytes()


def _streamer(dev):
    """the first two hops of a detector: its first step captures the launch chain, so the opt-ins happen inside a stream capture"""
    det = pkg.StreamingDetector(_model("simple", dev), n_mics=1, hop_samples=160)
    hops = pkg.synth.make_clips(3, 1, 320).reshape(1, 2, 160)
    out = []
    for k in range(2):
        det.step(torch.from_numpy(np.ascontiguousarray(hops[:, k])))
        det.stream.synchronize()
        out += [det.logits.cpu().numpy().tobytes(), det.prob.cpu().numpy().tobytes()]
    det.close()
    return b"".join(out)


def run(path: str) -> bytes:
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with torch.no_grad() if not path.startswith("train") else torch.enable_grad():
        if path == "frames_f16x3":
            return _forward(dev, "f16x3", 17408)
        if path == "frames_f32":
            return _forward(dev, "f32", 17408)
        if path == "pcm_f16x3d":
            return _forward(dev, "f16x3d", 16000)
        if path == "train3_f16x3":
            return _train(dev, "full", "f16x3")
        if path == "train2_f32":
            return _train(dev, "simple", "f32")
        if path == "augment":
            return _augment(dev)
        if path == "streamer":
            return _streamer(dev)
    raise ValueError(f"unknown path {path!r}: one of {PATHS}")


def digest(path: str) -> str:
    return hashlib.sha256(run(path)).hexdigest()


if __name__ == "__main__":
    print("FIRST_USE", sys.argv[1], digest(sys.argv[1]), int(nat.lib.ww_sync_timeouts()), flush=True)
