"""The bank audit restated on the host (include/wakeword_amd.h at ww_bank_audit_f32 is the definition): math.fsum for sums and frame
energies, numpy uint32 / uint64 for the hash, the activity rule as the header writes it.  Besides the fields it reports, per entry,
how close any frame's energy comes to the activity threshold: a test that compares extents exactly must first see that no frame of its
inputs sits within rounding of it."""
import math

import numpy as np

HOP = 512
M32 = np.uint64(0xFFFFFFFF)


def _fmix32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def mix(bits, index):
    """mix(bits, i) of the header, for arrays: bits uint32, index uint64 -> uint64."""
    bits = np.asarray(bits, np.uint32)
    index = np.asarray(index, np.uint64)
    lo = (index & M32).astype(np.uint32)
    hi = (index >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over="ignore"):
        m = lo * np.uint32(0x9E3779B1)
        k1 = bits ^ m ^ (hi * np.uint32(0x85EBCA77))
        rot = (m << np.uint32(15)) | (m >> np.uint32(17))
        k2 = bits + rot + hi * np.uint32(0xC2B2AE3D) + np.uint32(0x27D4EB2F)
        return _fmix32(k1).astype(np.uint64) | (_fmix32(k2).astype(np.uint64) << np.uint64(32))


def content_hash(x, first_index=0):
    """The wrapping uint64 sum of mix over the float32 samples x, the first of them at index `first_index` of its entry."""
    x = np.ascontiguousarray(x, np.float32)
    if x.size == 0:
        return 0
    with np.errstate(over="ignore"):
        return int(np.add.reduce(mix(x.view(np.uint32), np.arange(x.size, dtype=np.uint64) + np.uint64(first_index)), dtype=np.uint64))


def entry(x, ratio, clip_level):
    """One entry's record as a dict, from its float32 samples.  Extra keys: `abs_sum`, `abs_sumsq` (the sums of |terms|, for the float64
    summation bound) and `margin` (the smallest |E_t - E_max * ratio| / (E_max * ratio) over the frames; inf without a threshold)."""
    x = np.ascontiguousarray(x, np.float32)
    n = x.size
    finite = np.isfinite(x)
    xf = np.where(finite, x, np.float32(0)).astype(np.float64)
    sq = xf * xf                                                   # exact: a float32 square fits float64
    nh = -(-n // HOP)
    S = [math.fsum(sq[HOP * h:HOP * h + HOP]) for h in range(nh)]

    def block(h):
        return S[h] if 0 <= h < nh else 0.0
    E = [math.fsum([block(t - 2), block(t - 1), block(t), block(t + 1)]) for t in range(n // HOP + 1)]
    e_max = max(E)
    thr = e_max * ratio
    active = [t for t, v in enumerate(E) if e_max > 0 and v > thr]
    a, b = (HOP * active[0], min(n, HOP * (active[-1] + 1))) if active else (0, 0)
    nonfinite = int((~finite).sum())
    with np.errstate(invalid="ignore"):
        clipped = int((finite & (np.abs(x) >= np.float32(clip_level))).sum())
    if nonfinite:
        a, b = 0, n
    margin = min((abs(v - thr) / thr for v in E), default=math.inf) if e_max > 0 else math.inf
    return {"sum": math.fsum(xf), "sumsq": math.fsum(sq), "abs_sum": math.fsum(np.abs(xf)), "abs_sumsq": math.fsum(sq),
            "peak": np.fmax.reduce(np.abs(x), initial=np.float32(0)), "clipped": clipped,
            "nonfinite": nonfinite, "hash": content_hash(x), "max_frame_energy": e_max, "active_start": a, "active_end": b,
            "margin": margin}


def ratio_of(top_db):
    return 10.0 ** (-top_db / 10.0)
