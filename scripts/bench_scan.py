#!/usr/bin/env python3
"""Long-recording scan (scan.scan_files): hours of audio scored per second, with the decode, the windowed
forward and the 1,000-threshold event sweep timed apart.

    PYTHONPATH=. python scripts/bench_scan.py [--minutes 60] [--files 4] [--dir DIR] [--out profiles/scan_bench.json]

Inputs are generated from a seed into --dir (default: ww_scan_bench under the system's temporary directory; reused when present): --files PCM-16 16 kHz WAV files of --minutes of audio in all (noise with tone bursts), and
one FLAC file of a minute (tests/flacenc.py, the project's own encoder).  Every measurement reads them page-cached (one untimed pass
first).  Rows: window N of 16000 and 8000 samples, hops of 160 and 512.
  decode_s   decode_whole_file over every file (host read + upload + K0), synchronised
  forward_s  ww_forward_windows_f32 over the decoded, zero-padded signals (4096 windows per call), CUDA events
  scan_s     scan_files end to end (decode overlapped with the forward), wall clock
  sweep_s    Scan.counts at 1,000 thresholds (smooth 3, refractory 1 s): the smoothing and sweep kernels, wall clock around a sync"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import wakeword_jupyterlab_amd as pkg  # noqa: E402
from wakeword_jupyterlab_amd import _native as nat  # noqa: E402
from wakeword_jupyterlab_amd import scan  # noqa: E402
from wakeword_jupyterlab_amd.audio import decode_whole_file  # noqa: E402
from wakeword_jupyterlab_amd.files import WavBatchReader  # noqa: E402


def _ints(n, rng):
    t = np.arange(n) / 16000.0
    x = 0.05 * rng.standard_normal(n)
    burst = (np.sin(2 * np.pi * 0.37 * t) > 0.9)
    x += burst * 0.4 * np.sin(2 * np.pi * 523.0 * t)
    return np.clip(np.round(x * 32767), -32768, 32767).astype(np.int64)


def make_inputs(d, minutes, n_files, seed):
    import flacenc
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    per = int(minutes * 60 * 16000 / n_files)
    wavs = []
    for i in range(n_files):
        p = os.path.join(d, f"long{i}.wav")
        if not os.path.exists(p) or os.path.getsize(p) != 44 + 2 * per:
            with open(p, "wb") as f:
                f.write(flacenc.wav_bytes(_ints(per, rng), 16000, 16))
        wavs.append(p)
    flac = os.path.join(d, "long.flac")
    if not os.path.exists(flac):
        with open(flac, "wb") as f:
            f.write(flacenc.encode(_ints(60 * 16000, rng), 16000, 16))
    return wavs, flac


def _model(n, dev):
    cfg = type("Cfg", (pkg.AudioConfig,), {"DURATION": n / 16000.0})
    m = pkg.SimpleWakewordModel(audio_config=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in pkg.synth.make_state_dict("simple", seed=1234).items()})
    return m.to(dev).eval()


def time_decode(paths, dev):
    rd = WavBatchReader(max_clips=1, max_raw_bytes=1 << 22, slots=3, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = [decode_whole_file(rd, p, dev) for p in paths]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rd.close()
    return dt, out


def time_forward(m, signals, hop, dev, batch=4096):
    N = m._n_samples
    ws = torch.empty(nat.check(nat.lib.ww_forward_windows_workspace_bytes(batch, N, m._n_conv)), device=dev, dtype=torch.uint8)
    logits = torch.empty((batch, 2), device=dev)
    pads = []
    for x in signals:
        K = -(-x.numel() // hop)
        sig = torch.zeros(K * hop + N, device=dev)
        sig[N:N + x.numel()] = x
        pads.append((sig, K, torch.empty(K, device=dev)))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for sig, K, prob in pads:
        for b0 in range(0, K, batch):
            nb = min(batch, K - b0)
            nat.check(nat.lib.ww_forward_windows_f32(C.c_void_p(sig.data_ptr() + 4 * hop * (b0 + 1)), nb, hop, N, 1,
                                                     C.c_void_p(m.packed_weights().data_ptr()), m._n_conv, C.c_void_p(ws.data_ptr()),
                                                     ws.numel(), C.c_void_p(logits.data_ptr()), C.c_void_p(prob.data_ptr() + 4 * b0), stream))
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3, sum(K for _, K, _ in pads)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "ww_scan_bench"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    wavs, flac = make_inputs(args.dir, args.minutes, args.files, args.seed)
    hours = args.minutes / 60.0
    time_decode(wavs, dev)                                       # page cache + first-use costs
    dec_s, signals = time_decode(wavs, dev)
    fdec_s, fsig = time_decode([flac], dev)
    res = {"device": nat.device_info(), "audio_hours": hours, "files": len(wavs), "decode_s": dec_s,
           "decode_hours_per_s": hours / dec_s, "flac_minute_decode_s": fdec_s, "rows": []}
    thr = np.linspace(0.001, 1.0, 1000)
    for n in (16000, 8000):
        m = _model(n, dev)
        for hop in (160, 512):
            time_forward(m, signals[:1], hop, dev)               # warm-up
            fwd_s, n_win = time_forward(m, signals, hop, dev)
            scan.scan_files(m, wavs[:1], hop_samples=hop, keep_audio=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s = scan.scan_files(m, wavs, hop_samples=hop, keep_audio=False)
            scan_s = time.perf_counter() - t0
            s.counts(thr, smooth=3, refractory_s=1.0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.counts(thr, smooth=3, refractory_s=1.0)
            sweep_s = time.perf_counter() - t0
            row = {"window": n, "hop": hop, "windows": n_win, "forward_s": fwd_s, "windows_per_s": n_win / fwd_s,
                   "forward_hours_per_s": hours / fwd_s, "scan_s": scan_s, "scan_hours_per_s": hours / scan_s,
                   "scan_x_realtime": hours * 3600 / scan_s, "sweep_1000_s": sweep_s, "sweep_over_forward": sweep_s / fwd_s}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
