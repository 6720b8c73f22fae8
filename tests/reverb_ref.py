"""Float64 reference of the reverb stage ("Reverberation"), for the reverb tests.

    trim(h)             -> (kept taps, dpos): d = first index of max |h|, s = max(0, d - 40), kept = h[s : s + min(len - s, 16384)]
    reverb(x, kept, d)  -> y[i] = sum_k kept[k] x[i + d - k], i < N (x zero outside [0, N)), then out = sqrt(Ex / Ey) y
    decaying_rir(...)   -> the synthetic RIRs the tests use: silence, a direct-path spike after a pre-delay, exponentially decaying noise
"""
import numpy as np

MAX_TAPS = 16384
PRE_DIRECT = 40


def trim(h):
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    d = int(np.argmax(np.abs(h)))
    s = max(0, d - PRE_DIRECT)
    n = min(h.size - s, MAX_TAPS)
    return h[s:s + n], d - s


def convolve(x, kept, dpos):
    """The advanced linear convolution, no gain (float64)."""
    x = np.asarray(x, dtype=np.float64)
    kept = np.asarray(kept, dtype=np.float64)
    n = x.size
    size = 1 << int(np.ceil(np.log2(n + kept.size)))
    full = np.fft.irfft(np.fft.rfft(x, size) * np.fft.rfft(kept, size), size)[:n + kept.size - 1]
    return full[dpos:dpos + n]


def reverb(x, kept, dpos):
    x64 = np.asarray(x, dtype=np.float64)
    y = convolve(x64, kept, dpos)
    ex, ey = float((x64 ** 2).sum()), float((y ** 2).sum())
    return y * np.sqrt(ex / ey) if ex > 0 and ey > 0 else y


def decaying_rir(length, pre_delay, seed, rt_samples=2000.0, spike=1.0):
    """`length` taps: zeros for `pre_delay`, the direct path `spike` there, then noise decaying as exp(-t / rt_samples) (always below
    the spike in magnitude, so the direct path is the maximum)."""
    rng = np.random.default_rng(seed)
    h = np.zeros(length, dtype=np.float32)
    if pre_delay >= length:
        pre_delay = length - 1
    h[pre_delay] = spike
    t = np.arange(1, length - pre_delay, dtype=np.float64)
    if t.size:
        tail = rng.uniform(-0.6, 0.6, t.size) * np.exp(-t / rt_samples)
        h[pre_delay + 1:] = (tail * abs(spike)).astype(np.float32)
    return h
