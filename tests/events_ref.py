"""Numpy restatement of the event rule of INTEGRATION.md section 3f (smoothing, threshold, refractory period, FA/h, FRR), written from
the definitions for the tests: plain loops, float64 sums in ascending order."""
import math

import numpy as np


def smooth(p, w):
    """s_k = (sum_{j = max(1, k-w+1)}^{k} q_j) / (number of terms), q = p where finite else 0; float64, ascending j."""
    p = np.asarray(p, dtype=np.float32)
    q = np.where(np.isfinite(p), p, np.float32(0)).astype(np.float64)
    K = q.size
    k = np.arange(K)
    lo = np.maximum(0, k - w + 1)
    acc = np.zeros(K, np.float64)
    for t in range(w):                       # term t of window k is q[lo + t] while lo + t <= k: ascending j for every k
        j = lo + t
        ok = j <= k
        acc = np.where(ok, acc + q[np.minimum(j, max(K - 1, 0))], acc)
    return acc / (k - lo + 1).astype(np.float64)


def fired(s, thresholds, refractory):
    """[n_thr, K] bool: window k fires iff s_k >= (double)theta and k - k_last > R (or nothing fired before)."""
    th = np.asarray(thresholds, dtype=np.float32).astype(np.float64).reshape(-1)
    K = len(s)
    out = np.zeros((th.size, K), bool)
    last = np.full(th.size, -1, np.int64)
    have = np.zeros(th.size, bool)
    for k in range(K):
        f = (s[k] >= th) & (~have | (k - last > refractory))
        out[:, k] = f
        last = np.where(f, k, last)
        have |= f
    return out


def counts(p, offsets, thresholds, w, refractory):
    """[n_segs, n_thr] event counts of the segments prob[offsets[g]:offsets[g+1]]."""
    th = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    out = np.zeros((len(offsets) - 1, th.size), np.int64)
    for g in range(len(offsets) - 1):
        seg = np.asarray(p[offsets[g]:offsets[g + 1]])
        if seg.size:
            out[g] = fired(smooth(seg, w), th, refractory).sum(axis=1)
    return out


def refractory_windows(seconds, hop):
    return math.ceil(seconds * 16000 / hop)


def windows(x, n, hop):
    """The K = ceil(L / H) windows of x as rows [K, n]: window k (1-based) is x[kH - n, kH) with zeros outside x."""
    x = np.asarray(x, dtype=np.float32)
    K = -(-x.size // hop)
    pad = np.concatenate([np.zeros(n, np.float32), x, np.zeros(K * hop - x.size, np.float32)])
    return np.stack([pad[k * hop:k * hop + n] for k in range(1, K + 1)]) if K else np.zeros((0, n), np.float32)
