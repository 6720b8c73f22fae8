"""The weight-quantisation rule of include/wakeword_amd.h (ww_quant_weights_f32) restated in numpy float32, for the tests.

Every float32 step is one IEEE operation rounded to nearest -- numpy's float32 division and multiplication are --, np.rint rounds ties to
even, and subnormals are kept.  The error sums are float64: squares formed in float64 (exact products of float32 values need 48 bits, so
each square is rounded once) and added with math.fsum, i.e. the correctly rounded sum.  A kernel that adds the same float64 terms one by
one in any order is within (cols - 1) 2^-53 of it relative to the sum (all terms are non-negative), so `cols * 2^-52` bounds the
difference with room for the kernel's fused multiply-adds."""
import math

import numpy as np

TINY = np.float32(2.0 ** -126)


def qmax_of(bits: int) -> int:
    assert 2 <= bits <= 8
    return 2 ** (bits - 1) - 1


def quantize_rows(w2d: np.ndarray, bits: int = 8):
    """w2d float32 [rows, cols] -> dict(q int8, scale float32 [rows], deq float32, bad int32 [rows], err float64 [rows, 3])."""
    w = np.ascontiguousarray(w2d, dtype=np.float32)
    assert w.ndim == 2
    qmax = np.float32(qmax_of(bits))
    with np.errstate(all="ignore"):
        fin = np.isfinite(w)
        amax = np.where(fin, np.abs(w), np.float32(0)).astype(np.float32).max(axis=1)
        scale = np.maximum((amax / qmax).astype(np.float32), TINY).astype(np.float32)
        ratio = (np.where(fin, w, np.float32(0)).astype(np.float32) / scale[:, None]).astype(np.float32)
        r = np.clip(np.rint(ratio), -qmax, qmax)
        q = r.astype(np.int8)
        deq = (q.astype(np.float32) * scale[:, None]).astype(np.float32)
    bad = (~fin).sum(axis=1).astype(np.int32)
    err = np.zeros((w.shape[0], 3), np.float64)
    for i in range(w.shape[0]):
        wi = w[i][fin[i]].astype(np.float64)
        d = wi - deq[i][fin[i]].astype(np.float64)
        err[i, 0] = math.fsum(wi * wi)
        err[i, 1] = math.fsum(d * d)
        err[i, 2] = float(np.abs(d).max()) if d.size else 0.0
    return {"q": q, "scale": scale, "deq": deq, "bad": bad, "err": err}


def groups(shape, per_channel: bool = True):
    """(rows, cols) of a weight of this shape: ops.quant_groups."""
    n = int(np.prod(shape))
    if per_channel and len(shape) >= 2:
        return int(shape[0]), n // int(shape[0])
    return 1, n


def quantize(w: np.ndarray, bits: int = 8, per_channel: bool = True):
    """A weight of any shape: q and deq come back in that shape."""
    rows, cols = groups(w.shape, per_channel)
    out = quantize_rows(np.asarray(w, np.float32).reshape(rows, cols), bits)
    out["q"], out["deq"] = out["q"].reshape(w.shape), out["deq"].reshape(w.shape)
    return out


def fake_quant_state_dict(sd: dict, bits: int = 8, per_channel: bool = True, quantize_bias: bool = False) -> dict:
    """A model's state dict (numpy) with every weight replaced by its dequantised value, as quant.WeightQuant builds its model: tensors
    with two or more dimensions per row (or per tensor), one-dimensional ones only under quantize_bias, then per tensor."""
    out = {}
    for k, v in sd.items():
        v = np.asarray(v, np.float32)
        if v.ndim >= 2:
            out[k] = quantize(v, bits, per_channel)["deq"]
        elif quantize_bias:
            out[k] = quantize(v, bits, False)["deq"]
        else:
            out[k] = v.copy()
    return out
