"""numpy restatement of the microphone-channel stage as include/wakeword_amd.h states it: the counter-based
generator in uint64 arithmetic, the RBJ cookbook coefficients in float64, the cascade as a plain sequential direct-form recursion in a
chosen precision (float64: the reference; float32 with every operation rounded: the yardstick a float32 kernel is held to) and the
saturator.  Shared by tests/test_host_channel.py and tests/test_gpu_channel.py; nothing here touches the package."""
import numpy as np

from specaug_ref import word

FS = 16000.0
SECTIONS, RECORD = 8, 48
Q_BUTTERWORTH = 0.70710678118654752440

DEFAULTS = dict(prob=0.5, highpass_prob=0.5, highpass_hz=(20.0, 400.0), low_shelf_prob=0.5, low_shelf_hz=(100.0, 400.0), high_shelf_prob=0.5,
                high_shelf_hz=(2000.0, 5000.0), shelf_db=6.0, peaks=3, peak_prob=0.5, peak_hz=(100.0, 6000.0), peak_db=6.0, peak_q=(0.5, 2.0),
                lowpass_prob=0.3, lowpass_hz=(3000.0, 7500.0), drive_prob=0.2, drive=(0.5, 3.0))


def config_of(cfg) -> dict:
    """A config.ChannelConfig-like class as the keyword set of draw_records."""
    return {k: getattr(cfg, k.upper()) for k in DEFAULTS}


# ---- the generator ------------------------------------------------------------------------------------------------------------------
def on(seed, n, j, p) -> np.ndarray:
    """float(r >> 40) * 2^-24 < float32(p) for clips 0 .. n-1."""
    return (word(seed, n, j) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24) < np.float32(p)


def u53(seed, n, j) -> np.ndarray:
    return (word(seed, n, j) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def f32(v) -> np.float64:
    """A config scalar as the kernel sees it: rounded to float32, then widened."""
    return np.float64(np.float32(v))


def uniform(seed, n, j, lo, hi) -> np.ndarray:
    return f32(lo) + u53(seed, n, j) * (f32(hi) - f32(lo))


def log_uniform(seed, n, j, lo, hi) -> np.ndarray:
    return f32(lo) * np.power(f32(hi) / f32(lo), u53(seed, n, j))


# ---- the coefficients -----------------------------------------------------------------------------------------------------------------
def coefficients(kind, hz, db=0.0, q=Q_BUTTERWORTH) -> np.ndarray:
    """[..., 5] float64: b0, b1, b2, a1, a2 over a0 (RBJ "Audio EQ Cookbook" at 16 kHz), operation by operation as the kernel writes them."""
    hz, db, q = np.broadcast_arrays(np.asarray(hz, np.float64), np.asarray(db, np.float64), np.asarray(q, np.float64))
    w0 = 2.0 * 3.14159265358979323846 * hz / FS
    cs, alpha = np.cos(w0), np.sin(w0) / (2.0 * q)
    A = np.power(10.0, db / 40.0)
    if kind == "highpass":
        b0 = (1.0 + cs) / 2.0; b1 = -(1.0 + cs); b2 = b0
        a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha
    elif kind == "lowpass":
        b0 = (1.0 - cs) / 2.0; b1 = 1.0 - cs; b2 = b0
        a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha
    elif kind == "peak":
        b0 = 1.0 + alpha * A; b1 = -2.0 * cs; b2 = 1.0 - alpha * A
        a0 = 1.0 + alpha / A; a1 = -2.0 * cs; a2 = 1.0 - alpha / A
    else:
        t, ap, am = 2.0 * np.sqrt(A) * alpha, A + 1.0, A - 1.0
        if kind == "low_shelf":
            b0 = A * (ap - am * cs + t); b1 = 2.0 * A * (am - ap * cs); b2 = A * (ap - am * cs - t)
            a0 = ap + am * cs + t; a1 = -2.0 * (am + ap * cs); a2 = ap + am * cs - t
        elif kind == "high_shelf":
            b0 = A * (ap + am * cs + t); b1 = -2.0 * A * (am + ap * cs); b2 = A * (ap + am * cs - t)
            a0 = ap - am * cs + t; a1 = 2.0 * (am - ap * cs); a2 = ap - am * cs - t
        else:
            raise ValueError(kind)
    return np.stack([b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0], axis=-1)


def draw_records(seed, n, **kw):
    """(records float32 [n, 48], section flags bool [n, 8]) as ww_channel_draw writes them: the generator's table of section 3q."""
    c = dict(DEFAULTS, **kw)
    rec = np.zeros((n, RECORD), dtype=np.float64)
    rec[:, 0:5 * SECTIONS:5] = 1.0
    flags = np.zeros((n, SECTIONS), dtype=bool)
    clip = on(seed, n, 0, c["prob"])

    def put(slot, mask, co):
        mask = mask & clip
        flags[:, slot] = mask
        rec[mask, 5 * slot:5 * slot + 5] = co[mask]

    put(0, on(seed, n, 1, c["highpass_prob"]), coefficients("highpass", log_uniform(seed, n, 2, *c["highpass_hz"])))
    put(1, on(seed, n, 3, c["low_shelf_prob"]),
        coefficients("low_shelf", log_uniform(seed, n, 4, *c["low_shelf_hz"]), uniform(seed, n, 5, -np.float32(c["shelf_db"]), c["shelf_db"])))
    for i in range(int(c["peaks"])):
        j = 6 + 4 * i
        put(2 + i, on(seed, n, j, c["peak_prob"]),
            coefficients("peak", log_uniform(seed, n, j + 1, *c["peak_hz"]), uniform(seed, n, j + 2, -np.float32(c["peak_db"]), c["peak_db"]),
                         log_uniform(seed, n, j + 3, *c["peak_q"])))
    put(6, on(seed, n, 22, c["high_shelf_prob"]),
        coefficients("high_shelf", log_uniform(seed, n, 23, *c["high_shelf_hz"]), uniform(seed, n, 24, -np.float32(c["shelf_db"]), c["shelf_db"])))
    put(7, on(seed, n, 25, c["lowpass_prob"]), coefficients("lowpass", log_uniform(seed, n, 26, *c["lowpass_hz"])))
    drive = clip & on(seed, n, 27, c["drive_prob"])
    rec[drive, 5 * SECTIONS] = uniform(seed, n, 28, *c["drive"])[drive]
    return rec.astype(np.float32), flags


def is_identity(records) -> np.ndarray:
    """bool [n, 8]: the sections of a record that are [1, 0, 0, 0, 0]."""
    s = np.asarray(records)[:, :5 * SECTIONS].reshape(-1, SECTIONS, 5)
    return (s[:, :, 0] == 1) & (s[:, :, 1:] == 0).all(axis=2)


def is_off(records) -> np.ndarray:
    return is_identity(records).all(axis=1) & (np.asarray(records)[:, 5 * SECTIONS] == 0)


# ---- the filter -----------------------------------------------------------------------------------------------------------------------
def section(x, co, dtype) -> np.ndarray:
    """y[i] = b0 x[i] + b1 x[i-1] + b2 x[i-2] - a1 y[i-1] - a2 y[i-2], zero state, sample by sample in `dtype` (every operation rounded to
    it).  x [n, N]; co [n, 5].  The feed-forward sum does not depend on earlier outputs, so it is taken for all i at once, in the order
    ((b0 x + b1 x1) + b2 x2); the feedback runs in time order: (f - a1 y1) - a2 y2."""
    x = np.ascontiguousarray(np.asarray(x, dtype).T)                        # [N, n]: a sample of every clip per row
    b0, b1, b2, a1, a2 = (np.asarray(co[:, k], dtype) for k in range(5))
    x1, x2 = np.zeros_like(x), np.zeros_like(x)
    x1[1:], x2[2:] = x[:-1], x[:-2]
    with np.errstate(all="ignore"):
        f = b0 * x + b1 * x1 + b2 * x2
        y = np.empty_like(x)
        y1 = np.zeros(x.shape[1], dtype)
        y2 = np.zeros(x.shape[1], dtype)
        for i in range(x.shape[0]):
            v = f[i] - a1 * y1 - a2 * y2
            y[i] = v
            y2, y1 = y1, v
    assert y.dtype == dtype
    return np.ascontiguousarray(y.T)


def cascade(x, records, dtype=np.float64) -> np.ndarray:
    """The 8 sections of every clip's record, in slot order, on the float32 coefficients the record holds."""
    records = np.asarray(records, np.float32)
    y = np.asarray(x, np.float32).astype(dtype)
    ident = is_identity(records)
    for s in range(SECTIONS):
        act = ~ident[:, s]
        if act.any():
            y[act] = section(y[act], records[act, 5 * s:5 * s + 5], dtype)
    return y


def saturate(y, d, dtype=np.float64) -> np.ndarray:
    """out = p tanh(d y / p) / tanh(d), p = max |y| per clip; rows with d == 0 or p == 0 pass through."""
    y = np.asarray(y, dtype)
    d = np.asarray(d, dtype)
    out = y.copy()
    with np.errstate(all="ignore"):
        p = np.abs(y).max(axis=1)
        for r in np.flatnonzero((d != 0) & (p != 0)):
            out[r] = p[r] * np.tanh(d[r] * y[r] / p[r]) / np.tanh(d[r])
    assert out.dtype == dtype
    return out


def apply(x, records, dtype=np.float64) -> np.ndarray:
    """The whole stage in `dtype`: [n, N]."""
    records = np.asarray(records, np.float32)
    return saturate(cascade(x, records, dtype), records[:, 5 * SECTIONS], dtype)


def response(co, hz) -> np.ndarray:
    """|H(e^{jw})| of one section [5] (or the product over sections [k, 5]) at `hz`, float64."""
    co = np.atleast_2d(np.asarray(co, np.float64))
    z = np.exp(-1j * 2.0 * np.pi * np.float64(hz) / FS)
    h = (co[:, 0] + co[:, 1] * z + co[:, 2] * z * z) / (1.0 + co[:, 3] * z + co[:, 4] * z * z)
    return np.abs(np.prod(h))


def pole_radius(co) -> float:
    """The largest pole radius over the sections [k, 5]."""
    co = np.atleast_2d(np.asarray(co, np.float64))
    return max(float(np.abs(np.roots([1.0, c[3], c[4]])).max()) if (c[3] or c[4]) else 0.0 for c in co)
