"""Float64 restatements of ww_ce_loss_soft_f32 and ww_mixup_f32, the cases tests/test_gpu_mixup.py,
tests/test_host_mixup.py and scripts/soft_loss_errors.py share, and the caps on the REFERENCE's error that go with the rule of
tests/trainer_ref.py (`allowed`, U = 2^-24).  numpy only.

The error metrics are loss_ref's: the loss relative to its float64 value; the gradient as max |d - d64| * D / max(w), D being the mean's
denominator -- here the NUMBER of counted rows -- or 1 for a sum."""
import numpy as np

from loss_ref import REDUCTIONS, SIZES, SMOOTHINGS, WEIGHTS
from trainer_ref import U, ce_inputs

# Caps on torch's float32 error against this restatement: the next power of two at or above twice the largest figure that
# scripts/soft_loss_errors.py measured with torch on the CPU over every case of `soft_cases` (profiles/soft_loss_errors.json holds the
# figures: loss 2.07 u relative, gradient 5.33 u; u = 2^-24).  Never derived from the kernel's output; a GPU run records torch's
# figures on the device in the same file.
CAP_SOFT_LOSS, CAP_SOFT_DLOGITS = 8 * U, 16 * U

MIX_B, MIX_T = (1, 2, 5, 257), (1, 8, 31, 32)
# a mixed element: (1 - lam) * b rounded once, then one fused multiply-add rounded once -- at most two float32 roundings of magnitudes
# below 128, each at most 2^-24 * 128 = 7.6e-6; the float64 value itself uses the float32 (1 - lam), which is the specified weight
MIX_TOL = 1.6e-5


def soft_loss(logits, targets, weight=(1.0, 1.0), label_smoothing=0.0, reduction="mean"):
    """logits [n, 2], targets [n, 2] -> dict(loss, dlogits [n, 2], denom, max_w, correct, bad, counted) in float64:
    t' = (1 - eps) t + eps / 2;  l = sum_c w_c t'_c (lse - z_c);  dl/dz_k = p_k sum_c w_c t'_c - w_k t'_k.  A row counts iff both its
    targets are finite and >= 0; any other adds nothing to the loss, the gradient or the denominator and is counted in `bad`.  "mean"
    divides by the number of counted rows; a zero denominator gives a NaN loss and an all-zero gradient."""
    z = np.asarray(logits, np.float64)
    t = np.asarray(targets, np.float64)
    w = np.asarray(weight, np.float64)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(t).all(axis=1) & (t >= 0.0).all(axis=1)
    t = np.where(valid[:, None], t, 0.0)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(axis=1, keepdims=True)
    nlogp = (m + np.log(s)) - z
    p = e / s
    a = w * ((1.0 - label_smoothing) * t + 0.5 * label_smoothing)
    li = np.where(valid, (a * nlogp).sum(axis=1), 0.0)
    d = np.where(valid[:, None], p * a.sum(axis=1, keepdims=True) - a, 0.0)
    counted = int(valid.sum())
    denom = float(counted) if reduction == "mean" else 1.0
    pred = z[:, 1] > z[:, 0]
    out = {"denom": denom, "max_w": float(w.max()), "correct": int((valid & (pred == (t[:, 1] > t[:, 0]))).sum()),
           "bad": int((~valid).sum()), "counted": counted}
    if denom > 0.0:
        out["loss"], out["dlogits"] = float(li.sum() / denom), d / denom
    else:
        out["loss"], out["dlogits"] = float("nan"), np.zeros_like(d)
    return out


def soft_inputs(n, seed=None):
    """trainer_ref.ce_inputs' logits (|z| up to 160, ties, near ties, clips 3 and 4 at +-160) with float32 targets from a seeded draw:
    general rows (1 - t, t); every 6th row (from 1) un-normalised, two independent values in [0, 2); every 4th row (from 2) an exact
    one-hot, alternating the class; row 0 exactly (0.5, 0.5), a tie."""
    seed = 2000 + n if seed is None else seed
    z, _ = ce_inputs(n, seed=seed)
    rng = np.random.default_rng(seed + 1)
    u = rng.random(n).astype(np.float32)
    t = np.stack([np.float32(1.0) - u, u], axis=1)
    t[1::6] = (2.0 * rng.random((len(t[1::6]), 2))).astype(np.float32)
    hot = np.zeros((len(t[2::4]), 2), np.float32)
    hot[np.arange(len(hot)), np.arange(len(hot)) % 2] = 1.0
    t[2::4] = hot
    t[0] = (0.5, 0.5)
    return z, np.ascontiguousarray(t, dtype=np.float32)


def one_hot(labels):
    y = np.asarray(labels, np.int64)
    t = np.zeros((y.size, 2), np.float32)
    t[np.arange(y.size), y] = 1.0
    return t


def soft_cases(n):
    """The option sets of one size: weights x smoothing x reductions, as dict(tag, opts) with `opts` the keywords of ops.soft_ce_loss /
    mixup_ref.soft_loss."""
    return [{"tag": f"soft n={n} w={w} eps={eps} {red}", "opts": {"weight": w, "label_smoothing": eps, "reduction": red}}
            for w in WEIGHTS for eps in SMOOTHINGS for red in REDUCTIONS]


def restate(case, z, t):
    o = case["opts"]
    return soft_loss(z, t, o.get("weight") or (1.0, 1.0), o.get("label_smoothing", 0.0), o.get("reduction", "mean"))


def torch_reference(case, z, t, device, dtype=None):
    """torch's F.cross_entropy with probability targets on `device` (float32, or `dtype`): (loss as a float, dlogits as a numpy array)."""
    import torch
    import torch.nn.functional as F
    o = case["opts"]
    dtype = torch.float32 if dtype is None else dtype
    zt = torch.from_numpy(z).to(device=device, dtype=dtype).requires_grad_()
    tt = torch.from_numpy(t).to(device=device, dtype=dtype)
    w = None if o.get("weight") is None else torch.tensor(o["weight"], dtype=dtype, device=device)
    lt = F.cross_entropy(zt, tt, weight=w, label_smoothing=o.get("label_smoothing", 0.0), reduction=o.get("reduction", "mean"))
    lt.backward()
    return float(lt.detach()), zt.grad.detach().cpu().numpy()


# ---- mixup --------------------------------------------------------------------------------------------------------------------------
def mixup(mel, labels, partner, lam):
    """mel [B, ...] float32, labels [B] int64, partner [B] int32, lam [B] float32 -> (out float64 like mel, targets float32 [B, 2],
    mixed [B] bool).  A row is mixed iff lam != 1 and its partner lies in [0, B): out = lam * a + (1 - lam) * b with the float32
    (1 - lam), in float64; any other row is the input.  Targets are exact: NaN for a label outside {0, 1} on the row, a partner
    outside [0, B), or a label outside {0, 1} on a mixed row's partner; the one-hot when unmixed or both labels agree; else
    t[labels[i]] = lam, t[labels[p]] = 1 - lam."""
    mel = np.asarray(mel, np.float32)
    y, p, lam = np.asarray(labels, np.int64), np.asarray(partner, np.int64), np.asarray(lam, np.float32)
    B = mel.shape[0]
    out = mel.astype(np.float64)
    targets = np.full((B, 2), np.nan, np.float32)
    mixed = np.zeros(B, bool)
    for i in range(B):
        in_range = 0 <= p[i] < B
        mixed[i] = lam[i] != np.float32(1.0) and in_range
        oml = np.float32(1.0) - lam[i]
        if mixed[i]:
            out[i] = np.float64(lam[i]) * mel[i].astype(np.float64) + np.float64(oml) * mel[p[i]].astype(np.float64)
        if not in_range or y[i] not in (0, 1) or (mixed[i] and y[p[i]] not in (0, 1)):
            continue
        if not mixed[i] or y[p[i]] == y[i]:
            targets[i] = (1.0, 0.0) if y[i] == 0 else (0.0, 1.0)
        else:
            targets[i, y[i]], targets[i, y[p[i]]] = lam[i], oml
    return out, targets, mixed


def mix_inputs(B, T, seed=None):
    """Seeded mel values in [-80, 0] and a plan that covers the target rules: labels alternate by a seeded draw; a derangement-free
    random partner; lam 1 on about half the rows, else uniform in [0.5, 1); with B >= 5 row 1 carries label 7 and row 2 is mixed with it."""
    rng = np.random.default_rng(seed if seed is not None else 3000 + 64 * B + T)
    mel = (-80.0 * rng.random((B, 80, T))).astype(np.float32)
    labels = rng.integers(0, 2, B).astype(np.int64)
    partner = rng.permutation(B).astype(np.int32)
    lam = np.where(rng.random(B) < 0.5, 1.0, 0.5 + 0.5 * rng.random(B)).astype(np.float32)
    if B >= 2:
        lam[0] = 0.75                                     # at least one mixed row, exact in float32
        partner[0] = 1
    if B >= 5:
        labels[1] = 7                                     # a bad label on a row ...
        partner[2], lam[2] = 1, 0.625                     # ... and on the partner of a mixed row
        labels[3], labels[4] = 0, 1
        partner[3], lam[3] = 4, 0.875                     # different classes
        partner[4], lam[4] = 4, 0.5                       # its own partner: the same class
    return mel, labels, partner, lam
