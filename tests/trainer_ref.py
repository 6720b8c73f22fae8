"""Float64 restatements of what the trainer's kernels compute (cross-entropy over two classes, torch's single-tensor Adam,
clip_grad_norm_'s coefficient), the input recipe of the Adam tests and the tolerance rule they share.  numpy only.

The rule: the reference for a float32 quantity is torch's own float32 result on the same inputs; its error against the float64
restatement is measured inside the test and must stay under a fixed cap (so a bad input cannot hide a failure); ours may be at most
twice that plus one unit of 2^-24 -- the margin for an equally valid operation order and FMA contraction."""
import numpy as np

U = 2.0 ** -24
# caps on the REFERENCE's error (torch float32 against float64), in units of 2^-24 except the relative loss error
CAP_P, CAP_M, CAP_V = 16 * U, 2 * U, 1 * U
CAP_DLOGITS, CAP_LOSS = 4 * U, 2.0 ** -22


def allowed(ref_err: float) -> float:
    return 2.0 * ref_err + U


# ---- cross-entropy ----------------------------------------------------------------------------------------------------------------
def ce(logits, labels):
    """logits [n, 2], labels [n] -> (mean loss, dlogits [n, 2], correct) in float64.  A label outside {0, 1} adds nothing to loss or
    gradient (the mean still divides by n); the prediction is 1 iff z1 > z0."""
    z = np.asarray(logits, np.float64)
    y = np.asarray(labels, np.int64)
    n = z.shape[0]
    valid = (y == 0) | (y == 1)
    yc = np.where(valid, y, 0)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(axis=1, keepdims=True)
    lse = (m + np.log(s))[:, 0]
    loss = np.where(valid, lse - z[np.arange(n), yc], 0.0)
    onehot = np.zeros_like(z)
    onehot[np.arange(n), yc] = 1.0
    d = np.where(valid[:, None], (e / s - onehot) / n, 0.0)
    pred = (z[:, 1] > z[:, 0]).astype(np.int64)
    return float(loss.sum() / n), d, int(((pred == y) & valid).sum())


def ce_inputs(n, seed, labels="mixed"):
    """Logits with |z| up to 160, exact ties every 5th clip, near ties every 7th; labels mixed, all 0 or all 1."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((n, 2)) * rng.choice([0.1, 1.0, 10.0, 80.0], size=(n, 1))).astype(np.float32)
    z = np.clip(z, -160.0, 160.0)
    if n > 3:
        z[3] = (160.0, -160.0)
    if n > 4:
        z[4] = (-160.0, 160.0)
    z[::5, 1] = z[::5, 0]
    z[2::7, 1] = np.nextafter(z[2::7, 0], np.float32(np.inf))
    y = {"mixed": rng.integers(0, 2, n), "zeros": np.zeros(n), "ones": np.ones(n)}[labels].astype(np.int64)
    return z, y


# ---- Adam -------------------------------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, scale=1.0):
    """One update of torch's single-tensor Adam (no amsgrad, no maximize) in float64; returns (p, m, v, g') without touching the inputs."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    g = g * scale + weight_decay * p
    m = m + (g - m) * (1.0 - beta1)
    v = beta2 * v + (1.0 - beta2) * g * g
    c1, c2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    p = p - (lr / c1) * m / (np.sqrt(v) / np.sqrt(c2) + eps)
    return p, m, v, g


def adam_inputs(n, seed, steps=3):
    """The recipe: p0 = 0.1 N(0,1) with every 19th element exactly 0; g = N(0,1) 10^k, k uniform in -6..2 per element, every 7th 0,
    every 11th 1e-12 (the denominator is eps-dominated; its square is a normal float32), every 13th 1e4, every 17th with its sign
    flipped on step 2 (m cancels).  Returns p0 [n] and g [steps, n], float32."""
    rng = np.random.default_rng(seed)
    p0 = (0.1 * rng.standard_normal(n)).astype(np.float32)
    p0[::19] = 0.0
    g = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)).astype(np.float32)
    g[::7] = 0.0
    g[::11] = 1e-12
    g[::13] = 1e4
    gs = np.repeat(g[None], steps, axis=0)
    if steps > 1:
        gs[1, ::17] = -gs[1, ::17]
    return p0, gs


def adam_errors(p, m, v, p64, m64, v64, lr, gmax):
    """The three error metrics of the Adam tests: max |p - p64| / (|p64| + lr), max |m - m64| / gmax, max |v - v64| / gmax^2."""
    p, m, v = (np.asarray(a, np.float64) for a in (p, m, v))
    return (float(np.max(np.abs(p - p64) / (np.abs(p64) + lr))), float(np.max(np.abs(m - m64)) / gmax),
            float(np.max(np.abs(v - v64)) / gmax ** 2))


# ---- clip_grad_norm_ ----------------------------------------------------------------------------------------------------------------
def clip(grads, max_norm):
    """(global L2 norm, min(1, max_norm / (norm + 1e-6))) over a list of arrays, in float64."""
    norm = float(np.sqrt(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads)))
    return norm, min(1.0, max_norm / (norm + 1e-6))


# The bounds tests/test_gpu_trainer.py (test_grad_norm_and_clip_scale, test_max_grad_norm_clips_after_the_backward) holds ww_grad_norm_f32
# to, by name for the tests that check the norm of a composed step: the norm within 2^-22 of the float64 value, relative; an active
# scale within that plus one float32 rounding; an inactive one is exactly 1.
NORM_REL = 2.0 ** -22


def norm_bound(norm64: float) -> float:
    return NORM_REL * norm64


def scale_bound(scale64: float) -> float:
    return (NORM_REL + U) * scale64
