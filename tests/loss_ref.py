"""Float64 restatement of ww_ce_loss_ex_f32: cross-entropy with class weights, label smoothing, ignore_index
and a sum reduction, and the focal loss; the cases tests/test_gpu_loss.py, tests/test_host_loss.py and scripts/loss_errors.py share; and
the caps on the REFERENCE's error that go with the rule of tests/trainer_ref.py (`allowed`, U = 2^-24).  numpy only.

The error metrics: the loss relative to its float64 value; the gradient as max |d - d64| * D / max(w), D being the mean's denominator
(1 for a sum) -- trainer_ref's `* n` carried over to a weighted mean."""
import numpy as np

from trainer_ref import U, ce_inputs

# Caps on torch's float32 error against this restatement, per quantity: the next power of two at or above twice the largest figure that
# scripts/loss_errors.py measured with torch on the CPU over every case of `kernel_cases` (profiles/loss_errors.json holds the figures:
# cross-entropy loss 2.43 u relative and gradient 2.58 u; focal loss 2.59 u and gradient 832 u; u = 2^-24).  Never derived from the
# kernel's output; a GPU run records torch's figures on the device in the same file.  The focal gradient's figure is autograd's own
# cancellation in float32: at the clips where p_y -> 0 the backward of log_softmax subtracts gamma * 320 - 1 from gamma * 320.  The rule
# still holds the kernel to twice torch's error CASE BY CASE, so where torch is exact to a unit the kernel must be too.
CAP_CE_LOSS, CAP_CE_DLOGITS = 8 * U, 8 * U
CAP_FOCAL_LOSS, CAP_FOCAL_DLOGITS = 8 * U, 2048 * U

SIZES = (1, 2, 63, 64, 65, 257, 4099)
WEIGHTS = ((1.0, 1.0), (0.25, 4.0), (0.0, 1.0))
SMOOTHINGS = (0.0, 0.125)                                      # exact in float32: torch rounds label_smoothing to float32 internally
REDUCTIONS = ("mean", "sum")
LABELS = ("mixed", "zeros", "ones")
GAMMAS = (0.0, 0.5, 2.0, 5.0)


def loss(logits, labels, weight=(1.0, 1.0), label_smoothing=0.0, ignore_index=-100, reduction="mean", focal_gamma=None):
    """logits [n, 2], labels [n] -> dict(loss, dlogits [n, 2], denom, max_w, correct, bad, counted) in float64.  A clip whose label
    equals ignore_index (tested first) or lies outside {0, 1} adds nothing to the loss, the gradient or the denominator; the second kind
    is counted in `bad`.  A zero denominator under "mean" gives a NaN loss and an all-zero gradient."""
    z = np.asarray(logits, np.float64)
    y = np.asarray(labels, np.int64)
    n = z.shape[0]
    w = np.asarray(weight, np.float64)
    ignored = y == ignore_index
    valid = ~ignored & ((y == 0) | (y == 1))
    yc = np.where(valid, y, 0)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(axis=1, keepdims=True)
    logp = z - (m + np.log(s))
    p = e / s
    rows = np.arange(n)
    onehot = np.zeros_like(z)
    onehot[rows, yc] = 1.0
    wy = w[yc]
    if focal_gamma is None:
        eps = label_smoothing
        li = (1.0 - eps) * wy * -logp[rows, yc] + 0.5 * eps * (-logp * w).sum(axis=1)
        d = (1.0 - eps) * wy[:, None] * (p - onehot) + 0.5 * eps * (w.sum() * p - w)
        denom = float(wy[valid].sum()) if reduction == "mean" else 1.0
    else:
        g = focal_gamma
        py, q = p[rows, yc], p[rows, 1 - yc]
        qg = np.power(q, g)
        li = wy * qg * -logp[rows, yc]
        dy = wy * (g * py * qg * logp[rows, yc] - qg * q)
        d = np.where(onehot == 1.0, dy[:, None], -dy[:, None])
        denom = float(valid.sum()) if reduction == "mean" else 1.0
    li = np.where(valid, li, 0.0)
    d = np.where(valid[:, None], d, 0.0)
    pred = (z[:, 1] > z[:, 0]).astype(np.int64)
    out = {"denom": denom, "max_w": float(w.max()), "correct": int(((pred == y) & valid).sum()), "bad": int((~ignored & ~valid).sum()),
           "counted": int(valid.sum())}
    if denom > 0.0:
        out["loss"], out["dlogits"] = float(li.sum() / denom), d / denom
    else:
        out["loss"], out["dlogits"] = float("nan"), np.zeros_like(d)
    return out


def loss_error(value, want):
    """Relative error of a loss; 0 where both are the same number (a loss of exactly 0) or both are NaN."""
    if value != value or want != want:
        return 0.0 if (value != value and want != want) else float("inf")
    if value == want:
        return 0.0
    return abs(value - want) / abs(want) if want != 0.0 else float("inf")


def dlogits_error(d, want):
    """max |d - d64| * D / max(w)."""
    scale = (want["denom"] if want["denom"] > 0.0 else 1.0) / want["max_w"]
    return float(np.abs(np.asarray(d, np.float64) - want["dlogits"]).max()) * scale


def torch_labels(labels, ignore_index):
    """Labels as torch's own losses may be given them: a label outside {0, 1} other than ignore_index, which torch refuses, becomes
    ignore_index -- the same arithmetic: out of the loss, the gradient and the denominator."""
    y = np.asarray(labels, np.int64)
    return np.where((y == 0) | (y == 1) | (y == ignore_index), y, ignore_index)


def case_inputs(n, labels, extra=None):
    """trainer_ref.ce_inputs with every 11th label -100; extra="bad7" plants a label 7 (clip n // 2)."""
    z, y = ce_inputs(n, seed=1000 + n, labels=labels)
    y = y.copy()
    y[10::11] = -100
    if extra == "bad7":
        y[n // 2] = 7
    return z, y


def kernel_cases(n):
    """The option sets of one size, as dict(tag, labels, extra, opts) with `opts` the keywords of ops.ce_loss / loss_ref.loss:
    weights x smoothing x reduction x label mix for cross-entropy; ignore_index=1; a label 7; gamma x weights (x both reductions at
    gamma 2) for the focal loss, over the mixed labels whose clips 3 and 4 sit at +-160."""
    out = []
    for w in WEIGHTS:
        for eps in SMOOTHINGS:
            for red in REDUCTIONS:
                for lab in LABELS:
                    out.append({"tag": f"ce n={n} w={w} eps={eps} {red} {lab}", "labels": lab, "extra": None,
                                "opts": {"weight": w, "label_smoothing": eps, "reduction": red}})
    out.append({"tag": f"ce n={n} ignore_index=1", "labels": "mixed", "extra": None,
                "opts": {"weight": (0.25, 4.0), "label_smoothing": 0.125, "ignore_index": 1}})
    out.append({"tag": f"ce n={n} label 7", "labels": "mixed", "extra": "bad7", "opts": {"weight": (0.25, 4.0), "label_smoothing": 0.125}})
    for g in GAMMAS:
        for w in (None, (0.25, 4.0)):
            for red in (REDUCTIONS if g == 2.0 else ("mean",)):
                opts = {"focal_gamma": g, "reduction": red}
                if w is not None:
                    opts["weight"] = w
                out.append({"tag": f"focal n={n} gamma={g} w={w} {red}", "labels": "mixed", "extra": None, "opts": opts})
    out.append({"tag": f"focal n={n} label 7", "labels": "mixed", "extra": "bad7", "opts": {"focal_gamma": 2.0, "weight": (0.25, 4.0)}})
    return out


def restate(case, z, y):
    o = case["opts"]
    return loss(z, y, o.get("weight") or (1.0, 1.0), o.get("label_smoothing", 0.0), o.get("ignore_index", -100), o.get("reduction", "mean"),
                o.get("focal_gamma"))


def torch_reference(case, z, y, device, focal_cls):
    """torch's float32 loss and gradient on `device`: F.cross_entropy with the same options, or the expression of FocalLoss.forward.
    Returns (loss as a float, dlogits as a numpy array)."""
    import torch
    import torch.nn.functional as F
    o = case["opts"]
    ignore = o.get("ignore_index", -100)
    zt = torch.from_numpy(z).to(device).requires_grad_()
    yt = torch.from_numpy(torch_labels(y, ignore)).to(device)
    w = None if o.get("weight") is None else torch.tensor(o["weight"], dtype=torch.float32, device=device)
    if o.get("focal_gamma") is None:
        lt = F.cross_entropy(zt, yt, weight=w, label_smoothing=o.get("label_smoothing", 0.0), ignore_index=ignore,
                             reduction=o.get("reduction", "mean"))
    else:
        lt = focal_cls(o["focal_gamma"], weight=w, reduction=o.get("reduction", "mean"), ignore_index=ignore).to(device)(zt, yt)
    lt.backward()
    return float(lt.detach()), zt.grad.detach().cpu().numpy()
