"""Float64 numpy reference of loss-ranked selection (csrc/ww_select.hip): the per-clip losses, the three-key
order and the selection.  tests/loss_ref.py and tests/mixup_ref.py restate the same rules but return batch sums only, so the per-clip
forms are written out here and tests/test_host_select.py holds their sums to those two files (and to torch).  numpy only.

  score   the per-clip loss before the mean's division; -inf for a rank-0 row
  rank    2: a counting row of class keep_class with finite logits and a finite score; 1: any other such counting row; 0: the rest
  order   rank descending, score descending, row index ascending; the first `keep` rows, listed in rising row index"""
import numpy as np

OPTION_SETS = {                                                # the keywords of ops.loss_opts
    "default": {},
    "weights": {"weight": (1.0, 7.5)},
    "smoothing": {"label_smoothing": 0.1},
    "focal": {"focal_gamma": 2.0},
    "ignore": {"ignore_index": 1, "weight": (1.0, 7.5)},
}
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 65536)


def _lse_terms(logits):
    z = np.asarray(logits, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = z.max(axis=1, keepdims=True)
        lse = m + np.log(np.exp(z - m).sum(axis=1, keepdims=True))
        return z, lse - z                                      # -log p_c, [n, 2]


def label_losses(logits, labels, weight=(1.0, 1.0), label_smoothing=0.0, ignore_index=-100, focal_gamma=None, plain=False):
    """(loss float64 [n], counting bool [n], class int64 [n]) for integer labels.  `plain`: ww_ce_loss_f32's rule -- no options, and
    -100 is a bad label like any other outside {0, 1}.  A row that does not count has loss 0 here."""
    z, nlogp = _lse_terms(logits)
    y = np.asarray(labels, np.int64)
    w = np.asarray((1.0, 1.0) if plain else weight, np.float64)
    counting = (y == 0) | (y == 1)
    if not plain:
        counting &= y != ignore_index
    yc = np.where(counting, y, 0)
    rows = np.arange(z.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        if focal_gamma is None or plain:
            eps = 0.0 if plain else label_smoothing
            li = (1.0 - eps) * w[yc] * nlogp[rows, yc] + 0.5 * eps * (w * nlogp).sum(axis=1)
        else:
            li = w[yc] * np.exp(-focal_gamma * nlogp[rows, 1 - yc]) * nlogp[rows, yc]      # q^gamma from log q, q the OTHER class's term
    return np.where(counting, li, 0.0), counting, yc


def prob_losses(logits, targets, weight=(1.0, 1.0), label_smoothing=0.0):
    """The same for float32 class probabilities [n, 2]: a row counts iff both entries are finite and >= 0; its class is t1 > t0."""
    z, nlogp = _lse_terms(logits)
    t = np.asarray(targets, np.float64)
    w = np.asarray(weight, np.float64)
    with np.errstate(invalid="ignore"):
        counting = np.isfinite(t).all(axis=1) & (t >= 0.0).all(axis=1)
        tc = np.where(counting[:, None], t, 0.0)
        a = w * ((1.0 - label_smoothing) * tc + 0.5 * label_smoothing)
        li = (a * nlogp).sum(axis=1)
    return np.where(counting, li, 0.0), counting, (tc[:, 1] > tc[:, 0]).astype(np.int64)


def losses(logits, targets, opts=None):
    """Dispatch on the target's dtype; `opts` the keywords of ops.loss_opts / ops.soft_loss_opts, None for the plain rule."""
    t = np.asarray(targets)
    o = dict(opts or {})
    if t.dtype.kind == "f":
        return prob_losses(logits, t, o.get("weight") or (1.0, 1.0), o.get("label_smoothing", 0.0))
    if opts is None:
        return label_losses(logits, t, plain=True)
    return label_losses(logits, t, o.get("weight") or (1.0, 1.0), o.get("label_smoothing", 0.0), o.get("ignore_index", -100), o.get("focal_gamma"))


def ranks(logits, loss, counting, cls, keep_class=None):
    """Rank class per row, int64 [n]."""
    z = np.asarray(logits, np.float64)
    ranked = counting & np.isfinite(z).all(axis=1) & np.isfinite(loss)
    return np.where(ranked, np.where(cls == (-1 if keep_class is None else keep_class), 2, 1), 0).astype(np.int64)


def scores_of(loss, rank):
    return np.where(rank > 0, loss, -np.inf)


def order(scores, rank):
    """Row indices in the three-key order.  np.lexsort is stable and its LAST key is the primary one."""
    idx = np.arange(len(scores))
    with np.errstate(invalid="ignore"):
        return np.lexsort((idx, -np.asarray(scores, np.float64), -np.asarray(rank, np.int64)))


def select(scores, rank, keep):
    """The first `keep` rows of the order, in rising row index."""
    return np.sort(order(scores, rank)[:int(keep)])


def stats(scores, rank, counting, cls, sel):
    """One call's ww_select_stats as a dict (threshold as a float64)."""
    sel = np.asarray(sel, np.int64)
    positive = counting & (cls == 1)
    return {"batches": 1, "candidates": int(len(scores)), "kept": int(sel.size), "candidate_positive": int(positive.sum()),
            "kept_positive": int(positive[sel].sum()), "unranked": int((rank == 0).sum()), "kept_unranked": int((rank[sel] == 0).sum()),
            "threshold": float(np.asarray(scores, np.float64)[sel].min())}


def bound(logits, weight=(1.0, 1.0)):
    """The absolute error allowed per score: lse - z_y cancels, so 2^-46 max(1, |z0|, |z1|) (w0 + w1) -- about 64 float64 ulps of the
    largest intermediate."""
    z = np.abs(np.asarray(logits, np.float64))
    return 2.0 ** -46 * np.maximum(1.0, z.max(axis=1)) * float(np.sum(weight))


def random_inputs(n, scale, seed, soft=False):
    """float32 logits [n, 2] at `scale` and labels in {0, 1} (about one positive in four) -- or, `soft`, probability rows (1 - t, t)."""
    rng = np.random.default_rng(seed)
    z = (scale * rng.standard_normal((n, 2))).astype(np.float32)
    if soft:
        t1 = rng.random(n).astype(np.float32)
        return z, np.stack([np.float32(1.0) - t1, t1], axis=1)
    return z, (rng.random(n) < 0.25).astype(np.int64)


def grid_inputs(n, seed):
    """Inputs whose distinct losses are far apart: z = (0, m) with the signed margin s = m (2 y - 1) on a grid of 1/8 in [-8, 8), so a
    row's loss is softplus(-s) and two rows either are exact copies (same z, same y: a tie, broken by index) or differ by >= 4e-5.
    Returns (logits float32, labels int64, kind int64): rows of one `kind` are copies of one another."""
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < 0.25).astype(np.int64)
    step = 2 * rng.integers(-32, 32, n) + y                    # negatives on the even steps, positives on the odd ones: no margin is shared
    z = np.zeros((n, 2), np.float32)
    z[:, 1] = (step * (2 * y - 1)).astype(np.float32) / np.float32(8.0)
    return z, y, (step + 64) * 2 + y


def min_gap(loss, kind):
    """The smallest difference between the losses of two different kinds of row (inf with fewer than two kinds)."""
    _, first = np.unique(kind, return_index=True)
    v = np.sort(np.asarray(loss, np.float64)[first])
    return float(np.diff(v).min()) if v.size > 1 else float("inf")
