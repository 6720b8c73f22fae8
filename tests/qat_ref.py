"""The clipped quantisation rule of include/wakeword_amd.h (ww_quant_weights_clip_f32, ww_quant_clip_search_f32, ww_quant_ste_f32) restated
in numpy float32, for the tests: tests/quant_ref.py with a clip fraction per row.

Candidate j in 0 .. 47 has the fraction (64 - j) / 64, exact in float32; an index past 47 counts as 47.  Every float32 step is one IEEE
operation rounded to nearest, as in quant_ref.py, and the error sums are the correctly rounded float64 sums (math.fsum) of squares formed
in float64: a kernel that adds the same terms one by one is within `cols * 2^-52` of them, relative (quant_ref.py has the reasoning)."""
import math

import numpy as np

from quant_ref import TINY, groups, qmax_of

CLIP_STEPS = 48


def fractions(clip) -> np.ndarray:
    """float32 (64 - j) / 64 of the indices `clip`."""
    j = np.minimum(np.asarray(clip).astype(np.int64), CLIP_STEPS - 1)
    return ((64 - j).astype(np.float32) / np.float32(64)).astype(np.float32)


def _amax(w, fin):
    return np.where(fin, np.abs(w), np.float32(0)).astype(np.float32).max(axis=1)


def scales(w2d: np.ndarray, clip, bits: int) -> np.ndarray:
    """max((amax * f) / qmax, 2^-126) per row: one multiplication, one division."""
    w = np.ascontiguousarray(w2d, dtype=np.float32)
    qmax = np.float32(qmax_of(bits))
    with np.errstate(all="ignore"):
        amax = _amax(w, np.isfinite(w))
        return np.maximum(((amax * fractions(clip)).astype(np.float32) / qmax).astype(np.float32), TINY).astype(np.float32)


def _quantize(w, fin, scale, qmax):
    """(q int8, deq float32, moved bool) of rows `w` under one scale per row."""
    with np.errstate(all="ignore"):
        ratio = (np.where(fin, w, np.float32(0)).astype(np.float32) / scale[:, None]).astype(np.float32)
        r = np.rint(ratio)
        moved = np.abs(r) > qmax
        q = np.clip(r, -qmax, qmax).astype(np.int8)
        deq = (q.astype(np.float32) * scale[:, None]).astype(np.float32)
    return q, deq, moved


def quantize_rows_clip(w2d: np.ndarray, clip, bits: int = 8):
    """w2d float32 [rows, cols], clip [rows] -> dict(q, scale, deq, bad, sat int32 [rows], err float64 [rows, 3])."""
    w = np.ascontiguousarray(w2d, dtype=np.float32)
    assert w.ndim == 2 and len(clip) == w.shape[0]
    qmax = np.float32(qmax_of(bits))
    fin = np.isfinite(w)
    scale = scales(w, clip, bits)
    q, deq, moved = _quantize(w, fin, scale, qmax)
    err = np.zeros((w.shape[0], 3), np.float64)
    for i in range(w.shape[0]):
        wi = w[i][fin[i]].astype(np.float64)
        d = wi - deq[i][fin[i]].astype(np.float64)
        err[i] = math.fsum(wi * wi), math.fsum(d * d), float(np.abs(d).max()) if d.size else 0.0
    return {"q": q, "scale": scale, "deq": deq, "bad": (~fin).sum(axis=1).astype(np.int32), "sat": moved.sum(axis=1).astype(np.int32), "err": err}


def quantize_clip(w: np.ndarray, clip, bits: int = 8, per_channel: bool = True):
    """A weight of any shape: q and deq come back in that shape."""
    rows, cols = groups(w.shape, per_channel)
    out = quantize_rows_clip(np.asarray(w, np.float32).reshape(rows, cols), clip, bits)
    out["q"], out["deq"] = out["q"].reshape(w.shape), out["deq"].reshape(w.shape)
    return out


def search_rows(w2d: np.ndarray, bits: int = 8):
    """dict(cand_err float64 [rows, 48], clip uint8 [rows]: the first argmin, scale float32 [rows]: its scale, gap float64 [rows]: the
    relative distance of the second-best candidate's error from the best one's (inf when the best error is zero))."""
    w = np.ascontiguousarray(w2d, dtype=np.float32)
    rows = w.shape[0]
    qmax = np.float32(qmax_of(bits))
    fin = np.isfinite(w)
    cand = np.zeros((rows, CLIP_STEPS), np.float64)
    cand_scale = np.stack([scales(w, np.full(rows, j), bits) for j in range(CLIP_STEPS)], axis=1)
    for i in range(rows):
        wi, fi = w[i:i + 1], fin[i:i + 1]
        w64 = wi[0][fi[0]].astype(np.float64)
        for j in range(CLIP_STEPS):
            _, deq, _ = _quantize(wi, fi, cand_scale[i:i + 1, j], qmax)
            d = w64 - deq[0][fi[0]].astype(np.float64)
            cand[i, j] = math.fsum(d * d)
    clip = cand.argmin(axis=1).astype(np.uint8)              # numpy's argmin is the first
    two = np.sort(cand, axis=1)[:, :2]
    with np.errstate(all="ignore"):
        gap = np.where(two[:, 0] > 0.0, (two[:, 1] - two[:, 0]) / two[:, 0], np.inf)
    return {"cand_err": cand, "clip": clip, "scale": cand_scale[np.arange(rows), clip], "gap": gap}


def search(w: np.ndarray, bits: int = 8, per_channel: bool = True):
    rows, cols = groups(w.shape, per_channel)
    return search_rows(np.asarray(w, np.float32).reshape(rows, cols), bits)


def ste_rows(w2d: np.ndarray, scale: np.ndarray, g2d: np.ndarray, bits: int = 8) -> np.ndarray:
    """The straight-through estimator with clipping: g with +0.0 where w is finite and |rint(w / scale)| > qmax, its own bits elsewhere."""
    w = np.ascontiguousarray(w2d, dtype=np.float32)
    qmax = np.float32(qmax_of(bits))
    with np.errstate(all="ignore"):
        moved = np.isfinite(w) & (np.abs(np.rint((w / np.asarray(scale, np.float32)[:, None]).astype(np.float32))) > qmax)
    out = np.array(g2d, dtype=np.float32, copy=True)
    out[moved] = np.float32(0.0)
    return out


def ste(w: np.ndarray, scale: np.ndarray, g: np.ndarray, bits: int = 8, per_channel: bool = True) -> np.ndarray:
    rows, cols = groups(w.shape, per_channel)
    return ste_rows(np.asarray(w, np.float32).reshape(rows, cols), scale, np.asarray(g, np.float32).reshape(rows, cols), bits).reshape(w.shape)


def fake_quant_clip_state_dict(sd: dict, clips: dict, bits: int = 8, per_channel: bool = True) -> dict:
    """quant_ref.fake_quant_state_dict under clip indices {name: [rows]} for the tensors with two or more dimensions; the rest as they are."""
    return {k: quantize_clip(np.asarray(v, np.float32), clips[k], bits, per_channel)["deq"] if np.ndim(v) >= 2 else np.asarray(v, np.float32).copy()
            for k, v in sd.items()}
