"""Float64 restatement of ww_distill_loss_f32: Hinton's distillation loss over two classes,

    L = (1 - alpha) H(z, y) + alpha T^2 KD(z, zt),   KD_i = sum_c q_c (log q_c - log p_c),  q = softmax(zt_i / T),  p = softmax(z_i / T)
    dKD_i / dz_k = (p_k - q_k) / T

its gradient and both device records; the inputs and option sets tests/test_gpu_distill.py, tests/test_host_distill.py and
scripts/distill_errors.py share; and the two bounds of the issue.  numpy only.  The hard term H is the restatement that already exists
for its rule: loss_ref.loss for integer labels (ww_ce_loss_ex_f32), mixup_ref.soft_loss for class probabilities (ww_ce_loss_soft_f32).

The bounds (a float64 result rounded to float32 once, plus the float64 cancellation in p - q):
    |loss - ref| <= 2^-23 |ref| + 1e-12
    |d - ref|    <= 2^-23 |ref| + 1e-12 * (alpha T / D_kd + (1 - alpha) max(w, 1) / D_hard)
with each part of the absolute term over its own term's denominator (a part whose term is absent or empty is left out)."""
import numpy as np

import loss_ref
import mixup_ref

EPS32 = 2.0 ** -23
SIZES = (1, 2, 3, 255, 256, 257, 511, 512, 513, 1025)
TEMPERATURES = (0.05, 1.0, 2.0, 20.0)
ALPHAS = (0.0, 0.3, 1.0)


def _log_softmax(a):
    m = a.max(axis=1, keepdims=True)
    e = np.exp(a - m)
    s = e.sum(axis=1, keepdims=True)
    return a - (m + np.log(s)), e / s


def _kind(targets):
    if targets is None:
        return "none"
    return "probs" if np.asarray(targets).dtype.kind == "f" else "labels"


def distill(logits, teacher, targets=None, alpha=0.5, temperature=2.0, weight=None, label_smoothing=0.0, ignore_index=-100,
            reduction="mean", focal_gamma=None):
    """logits, teacher [n, 2]; targets None, int64 [n] or float32 [n, 2] -> dict in float64:
      loss, dlogits          the batch's L and dL/dz (NaN and zeros when, under the mean, neither term has a counted row)
      hard, kd               H and T^2 KD, each over its own denominator, not weighted by alpha (0 for a term without a counted row)
      hard_denom, kd_denom   the two denominators (1 under the sum; hard_denom 0 without a target)
      abs_scale              the factor of the gradient bound's absolute part
      stats                  what the call adds to ww_loss_stats but for loss_sum: correct, total, bad_labels, nonfinite
      dstats                 what it adds to ww_distill_stats but for the two sums"""
    z = np.asarray(logits, np.float64)
    zt = np.asarray(teacher, np.float64)
    n, T, mean = z.shape[0], float(temperature), reduction == "mean"
    w = (1.0, 1.0) if weight is None else weight
    kind = _kind(targets)
    pred, pred_t = z[:, 1] > z[:, 0], zt[:, 1] > zt[:, 0]

    # ---- the teacher term ----
    rows = np.isfinite(zt).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        logq, q = _log_softmax(np.where(rows[:, None], zt, 0.0) / T)
        logp, p = _log_softmax(z / T)
        kd_i = np.where(rows, (q * (logq - logp)).sum(axis=1), 0.0)
        dkd = np.where(rows[:, None], (p - q) / T, 0.0)
    kd_rows = int(rows.sum())
    kd_denom = float(kd_rows) if mean else 1.0
    kd_has = kd_denom > 0.0

    # ---- the hard term: the existing restatement of its rule, as a sum and with the mean's denominator ----
    stats = {"correct": 0, "total": n, "bad_labels": 0, "nonfinite": int((~np.isfinite(z).all(axis=1)).sum())}
    hard_rows = teacher_correct = 0
    hard_denom, hard_sum, dhard, max_w = 0.0, 0.0, np.zeros_like(z), 1.0
    if kind == "labels":
        y = np.asarray(targets, np.int64)
        s = loss_ref.loss(z, y, w, label_smoothing, ignore_index, "sum", focal_gamma)
        hard_denom = loss_ref.loss(z, y, w, label_smoothing, ignore_index, reduction, focal_gamma)["denom"]
        valid = (y != ignore_index) & ((y == 0) | (y == 1))
        teacher_correct = int((valid & (pred_t == (y == 1))).sum())
    elif kind == "probs":
        t = np.asarray(targets, np.float32)
        s = mixup_ref.soft_loss(z, t, w, label_smoothing, "sum")
        hard_denom = mixup_ref.soft_loss(z, t, w, label_smoothing, reduction)["denom"]
        with np.errstate(invalid="ignore"):
            valid = np.isfinite(t).all(axis=1) & (t >= 0.0).all(axis=1)
            teacher_correct = int((valid & (pred_t == (t[:, 1] > t[:, 0]))).sum())
    if kind != "none":
        hard_sum, dhard, max_w, hard_rows = s["loss"], s["dlogits"], max(s["max_w"], 1.0), s["counted"]
        stats["correct"], stats["bad_labels"] = s["correct"], s["bad"]
    hard_has = hard_denom > 0.0
    ch, ck = (0.0, 1.0) if kind == "none" else (1.0 - alpha, float(alpha))

    hard = hard_sum / hard_denom if hard_has else 0.0
    kd = T * T * (kd_i.sum() / kd_denom) if kd_has else 0.0
    d = np.zeros_like(z)
    loss, abs_scale = 0.0, 0.0
    if hard_has and ch > 0.0:
        loss += ch * hard
        d += ch * dhard / hard_denom
        abs_scale += ch * max_w / hard_denom
    if kd_has and ck > 0.0:
        loss += ck * kd
        d += ck * T * T * dkd / kd_denom
        abs_scale += ck * T / kd_denom
    if not hard_has and not kd_has:
        loss, d = float("nan"), np.zeros_like(z)
    return {"loss": float(loss), "dlogits": d, "hard": float(hard), "kd": float(kd), "hard_denom": hard_denom, "kd_denom": kd_denom,
            "abs_scale": abs_scale, "stats": stats,
            "dstats": {"kd_rows": kd_rows, "hard_rows": int(hard_rows), "agree": int((rows & (pred == pred_t)).sum()),
                       "teacher_correct": teacher_correct, "teacher_nonfinite": n - kd_rows}}


def loss_bound(want):
    return EPS32 * abs(want) + 1e-12


def dlogits_bound(want):
    """The per-element bound, an array like want["dlogits"]."""
    return EPS32 * np.abs(want["dlogits"]) + 1e-12 * want["abs_scale"]


def loss_excess(value, want):
    """|value - want| - bound (<= 0 passes); -inf where both are NaN, +inf where one is."""
    if value != value or want != want:
        return float("-inf") if (value != value and want != want) else float("inf")
    return abs(value - want) - loss_bound(want)


def dlogits_excess(d, want):
    return float((np.abs(np.asarray(d, np.float64) - want["dlogits"]) - dlogits_bound(want)).max())


# ---- inputs and option sets ------------------------------------------------------------------------------------------------------------
def inputs(n, seed=None, nonfinite_teacher=True):
    """Seeded float32 student and teacher logits with |z| up to 80: scales 0.1 .. 40 per row, row 3 / 4 at +-80 on both sides (agreeing
    and opposed), exact ties every 5th student row and every 9th teacher row, near ties every 7th; a teacher that follows the student on
    every third row; int64 labels with every 11th -100 and one label 7; float32 probabilities (mixup_ref.soft_inputs' recipe) with a NaN row.
    With `nonfinite_teacher`, teacher row 1 is (Inf, 0) and row 6 (NaN, NaN)."""
    seed = 7000 + n if seed is None else seed
    rng = np.random.default_rng(seed)
    z = np.clip(rng.standard_normal((n, 2)) * rng.choice([0.1, 1.0, 10.0, 40.0], size=(n, 1)), -80.0, 80.0).astype(np.float32)
    zt = np.clip(rng.standard_normal((n, 2)) * rng.choice([0.1, 1.0, 10.0, 40.0], size=(n, 1)), -80.0, 80.0).astype(np.float32)
    zt[::3] = (z[::3] * np.float32(1.25)).astype(np.float32)
    if n > 3:
        z[3], zt[3] = (80.0, -80.0), (80.0, -80.0)
    if n > 4:
        z[4], zt[4] = (-80.0, 80.0), (80.0, -80.0)
    z[::5, 1] = z[::5, 0]
    zt[::9, 1] = zt[::9, 0]
    z[2::7, 1] = np.nextafter(z[2::7, 0], np.float32(np.inf))
    if nonfinite_teacher:
        if n > 1:
            zt[1] = (np.inf, 0.0)
        if n > 6:
            zt[6] = (np.nan, np.nan)
    y = rng.integers(0, 2, n).astype(np.int64)
    y[10::11] = -100
    if n > 8:
        y[8] = 7
    _, t = mixup_ref.soft_inputs(n, seed=seed + 1)
    if n > 5:
        t[5] = (np.nan, np.nan)
    return z, zt, y, t


# (tag, the kind of target, the keywords of ops.distill_loss / distill_ref.distill but for alpha and temperature)
OPTION_SETS = (
    ("labels", "labels", {}),
    ("labels w eps", "labels", {"weight": (0.25, 4.0), "label_smoothing": 0.125}),
    ("labels ignore 1 sum", "labels", {"weight": (0.25, 4.0), "ignore_index": 1, "reduction": "sum"}),
    ("labels focal", "labels", {"focal_gamma": 2.0, "weight": (0.25, 4.0)}),
    ("labels focal sum", "labels", {"focal_gamma": 0.5, "reduction": "sum"}),
    ("probs", "probs", {}),
    ("probs w eps sum", "probs", {"weight": (0.25, 4.0), "label_smoothing": 0.125, "reduction": "sum"}),
    ("probs w", "probs", {"weight": (0.0, 1.0)}),
    ("none", "none", {}),
    ("none sum", "none", {"reduction": "sum"}),
)


def grid():
    """(tag, kind, opts, alpha, temperature) over OPTION_SETS x ALPHAS x TEMPERATURES; without a target alpha is not read: one value."""
    for tag, kind, opts in OPTION_SETS:
        for alpha in (ALPHAS if kind != "none" else (0.3,)):
            for T in TEMPERATURES:
                yield f"{tag} alpha={alpha} T={T}", kind, opts, alpha, T


def target_of(kind, y, t):
    return {"labels": y, "probs": t, "none": None}[kind]


def torch_formula(z, zt, target, alpha, T, opts, device, dtype, focal_cls):
    """The same loss composed from torch's own pieces in `dtype` on `device`, with autograd's gradient: (loss as a float, dlogits as a
    numpy array).  Rows that do not count are taken out by indexing; an empty term is left out."""
    import torch
    import torch.nn.functional as F
    zz = torch.from_numpy(np.asarray(z)).to(device=device, dtype=dtype).requires_grad_()
    tt = torch.from_numpy(np.asarray(zt)).to(device=device, dtype=dtype)
    mean = opts.get("reduction", "mean") == "mean"
    w = None if opts.get("weight") is None else torch.tensor(opts["weight"], dtype=dtype, device=device)
    rows = torch.isfinite(tt).all(dim=1)
    total = zz.sum() * 0.0
    ck = 1.0 if target is None else alpha
    if rows.any() and ck > 0.0:
        kd = F.kl_div(F.log_softmax(zz[rows] / T, dim=1), F.softmax(tt[rows] / T, dim=1), reduction="batchmean" if mean else "sum") * T * T
        total = total + ck * kd
    if target is not None and alpha < 1.0:
        tg = torch.from_numpy(np.asarray(target)).to(device)
        if tg.dtype.is_floating_point:
            valid = torch.isfinite(tg).all(dim=1) & (tg >= 0).all(dim=1)
            if valid.any():
                h = F.cross_entropy(zz[valid], tg[valid].to(dtype), weight=w, label_smoothing=opts.get("label_smoothing", 0.0), reduction="sum")
                total = total + (1.0 - alpha) * (h / valid.sum() if mean else h)
        else:
            ignore = opts.get("ignore_index", -100)
            valid = (tg != ignore) & ((tg == 0) | (tg == 1))
            if valid.any():
                if opts.get("focal_gamma") is None:
                    h = F.cross_entropy(zz[valid], tg[valid], weight=w, label_smoothing=opts.get("label_smoothing", 0.0),
                                        reduction=opts.get("reduction", "mean"))
                else:
                    h = focal_cls(opts["focal_gamma"], weight=w, reduction=opts.get("reduction", "mean")).to(device)(zz[valid], tg[valid])
                if bool(torch.isfinite(h)) or not mean:
                    total = total + (1.0 - alpha) * h
    total.backward()
    return float(total.detach()), zz.grad.detach().cpu().numpy()
