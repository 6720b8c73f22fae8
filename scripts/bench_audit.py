#!/usr/bin/env python3
"""Bank audit: ww_bank_audit_f32 over a one-hour bank of 1 s to 3 s entries against ww_bank_peaks_f32 over the
same buffer and table -- the kernel that read these bytes before the audit existed.

    PYTHONPATH=. python scripts/bench_audit.py [--hours 1] [--calls 40] [--out profiles/audit_bench.json]

Both calls alternate call for call with a device event pair around each; buffers, table and workspace are allocated once.  The audit's
time is both of its kernels and the staging of its hop table.  The ratio has no required value: the audit runs once per bank, beside
a decode that takes far longer; it is recorded so that the cost of the content hash is known and a later change can be judged."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from wakeword_jupyterlab_amd import _native as nat  # noqa: E402
from wakeword_jupyterlab_amd.audit import STATS_DTYPE, top_db_ratio  # noqa: E402

RATE = 16000
HBM_PEAK = 8.0e12          # bytes/s, the card's specified peak


def _timed_pairs(fns, calls):
    """Each function `calls` times, alternating call for call, a device event pair around every call -> ms lists."""
    ms = [[] for _ in fns]
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(calls):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            pairs.append((k, a, b))
    torch.cuda.synchronize()
    for k, a, b in pairs:
        ms[k].append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--out", default=os.path.join("profiles", "audit_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    total = int(a.hours * 3600 * RATE)
    rng = np.random.default_rng(0)
    lengths = []
    left = total
    while left > 0:                                                  # entries of 1 s to 3 s, any sample count, until the hour is full
        n = min(left, int(rng.integers(RATE, 3 * RATE + 1)))
        lengths.append(n)
        left -= n
    table = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = len(lengths)
    data = torch.randn(total, device=dev) * 0.1
    off = torch.from_numpy(table).to(dev)
    peaks = torch.empty(n, device=dev)
    stats = torch.empty(n * STATS_DTYPE.itemsize, device=dev, dtype=torch.uint8)
    ws = torch.empty(nat.check(nat.lib.ww_bank_audit_workspace_bytes(total, n)), device=dev, dtype=torch.uint8)
    ratio = top_db_ratio(60.0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

    def audit():
        nat.check(nat.lib.ww_bank_audit_f32(p(data), total, p(off), table.ctypes.data, n, 0.999, ratio, p(stats), p(ws), stream))

    def peak():
        nat.check(nat.lib.ww_bank_peaks_f32(p(data), total, p(off), n, p(peaks), stream))

    t_audit, t_peak = _timed_pairs([audit, peak], a.calls)
    got = stats.cpu().numpy().view(STATS_DTYPE)
    assert np.array_equal(got["peak"].view(np.uint32), peaks.cpu().numpy().view(np.uint32))
    ma, mp = statistics.median(t_audit), statistics.median(t_peak)
    nbytes = 4 * total
    res = {"device": nat.device_info(), "hbm_peak_bytes_per_s": HBM_PEAK, "samples": total, "entries": n, "entry_seconds": [1, 3],
           "bytes": nbytes, "calls": a.calls,
           "audit_ms_median": ma, "audit_ms_min": min(t_audit), "audit_ms_mean": statistics.fmean(t_audit),
           "peaks_ms_median": mp, "peaks_ms_min": min(t_peak), "peaks_ms_mean": statistics.fmean(t_peak),
           "audit_bytes_per_s": nbytes / (ma * 1e-3), "peaks_bytes_per_s": nbytes / (mp * 1e-3),
           "audit_share_of_hbm_peak": nbytes / (ma * 1e-3) / HBM_PEAK, "peaks_share_of_hbm_peak": nbytes / (mp * 1e-3) / HBM_PEAK,
           "audit_over_peaks": ma / mp, "hash": "two 32-bit finalisers per sample (include/wakeword_amd.h)"}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
