"""FLAC against WAV through the file-fed reader: the same 4096 one-second 16 kHz mono clips (create_sample_data's recipe: PCM-16) written
once as WAV and once as FLAC (tests/flacenc.py: FIXED / Rice subframes, 4096-sample frames, what a default encoder writes for such
content), then streamed through WavBatchReader.stream in batches of 4096 -- host threads, H2D, (FLAC decode kernel,) K0 -- in files/s,
WAV and FLAC passes interleaved.  A host-only reader times the threaded part alone (open, read, RIFF walk or FLAC sync scan + CRCs)
per file and thread.

    PYTHONPATH=. python scripts/bench_flac.py [--passes 8] [--out profiles/flac_bench.json]
Under `rocprofv3 --kernel-trace --stats -- python scripts/bench_flac.py` the FLAC kernel's time per 4096 clips is in the stats."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_sets(d, n=4096, distinct=64):
    import flacenc
    import wakeword_jupyterlab_amd as pkg
    wav, flac, fbytes, wbytes = [], [], 0, 0
    enc = []
    for i in range(distinct):
        x = np.clip(np.round(pkg.synth.make_clip(i) * 32767), -32768, 32767).astype(np.int64)
        enc.append((flacenc.wav_bytes(x, 16000, 16), flacenc.encode(x, 16000, 16, subframe="fixed", order=2)))
    for i in range(n):
        w, f = enc[i % distinct]
        for lst, data, ext in ((wav, w, "wav"), (flac, f, "flac")):
            p = os.path.join(d, f"c{i:05d}.{ext}")
            with open(p, "wb") as fh:
                fh.write(data)
            lst.append(p)
        wbytes += len(w)
        fbytes += len(f)
    return wav, flac, wbytes / n, fbytes / n


def stream_rate(paths, batch, passes):
    from wakeword_jupyterlab_amd import files
    rd = files.WavBatchReader(max_clips=batch, max_raw_bytes=batch * 70000, slots=3)
    enc = files.EncodedPaths(paths)
    for out, ok in rd.stream(enc, batch, verbose=False):        # warm-up: page cache, the slots' device regions
        assert ok.all()
    torch.cuda.synchronize()
    rates = []
    for _ in range(passes):
        t0 = time.perf_counter()
        for out, ok in rd.stream(enc, batch, verbose=False):
            pass
        torch.cuda.synchronize()
        rates.append(len(paths) / (time.perf_counter() - t0))
    rd.close()
    return rates


def host_us_per_file(paths, threads, reps=5):
    """The reader threads' part alone (host-only reader): us per file per thread."""
    from wakeword_jupyterlab_amd import files
    rd = files.WavBatchReader(max_clips=len(paths), max_raw_bytes=len(paths) * 70000, threads=threads, host_only=True)
    enc = files.EncodedPaths(paths)
    rd.read(enc, 0)
    best = []
    for _ in range(reps):
        t0 = time.perf_counter()
        _, st = rd.read(enc, 0)
        best.append((time.perf_counter() - t0) * threads / len(paths) * 1e6)
        assert (st == 1).all()
    rd.close()
    return float(np.median(best))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from wakeword_jupyterlab_amd import files
    d = tempfile.mkdtemp(prefix="ww_flac_bench_")
    try:
        wav, flac, wb, fb = make_sets(d, args.batch)
        res = {"files": args.batch, "wav_bytes_per_file": wb, "flac_bytes_per_file": fb, "reader_threads": files.default_threads()}
        for th in (1, files.default_threads()):
            res[f"host_us_per_file_per_thread_wav_t{th}"] = host_us_per_file(wav, th)
            res[f"host_us_per_file_per_thread_flac_t{th}"] = host_us_per_file(flac, th)
        w, f = [], []
        for _ in range(2):                                          # interleaved
            w += stream_rate(wav, args.batch, args.passes // 2)
            f += stream_rate(flac, args.batch, args.passes // 2)
        res.update(wav_files_per_s_median=float(np.median(w)), flac_files_per_s_median=float(np.median(f)),
                   wav_files_per_s=[round(x) for x in w], flac_files_per_s=[round(x) for x in f])
        res["flac_over_wav"] = res["flac_files_per_s_median"] / res["wav_files_per_s_median"]
        res["flac_errors"] = files.flac_errors()
        line = json.dumps(res)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
