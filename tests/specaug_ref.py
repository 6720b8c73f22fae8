"""numpy restatement of SpecAugment as include/wakeword_amd.h states it: the counter-based generator in
uint64 arithmetic, exact, and the masking with the clip's mean taken in float64.  Shared by tests/test_host_specaug.py and
tests/test_gpu_specaug.py; nothing here touches the package."""
import numpy as np

N_MELS = 80
GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def fmix64(x: np.ndarray) -> np.ndarray:
    """The three xor-shift-multiply steps of splitmix64 on a uint64 array (wrapping)."""
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def word(seed: int, n: int, j: int) -> np.ndarray:
    """r(c, j) for c = 0 .. n-1."""
    with np.errstate(over="ignore"):
        c = np.arange(n, dtype=np.uint64)
        return fmix64(np.uint64(int(seed) & M64) + np.uint64(GOLDEN) * (np.uint64(32) * c + np.uint64(j + 1)))


def int_in(r: np.ndarray, m) -> np.ndarray:
    """((r >> 32) * (m + 1)) >> 32: an integer in 0 .. m (m a scalar or an array)."""
    return ((r >> np.uint64(32)) * (np.asarray(m, dtype=np.uint64) + np.uint64(1))) >> np.uint64(32)


def time_max(fraction: float, T: int) -> int:
    return int(float(fraction) * T)


def draw_records(seed: int, n: int, T: int, prob: float = 0.8, n_freq: int = 2, freq_max: int = 12, n_time: int = 2, t_max=None,
                 fraction: float = 0.125) -> np.ndarray:
    """int16 [n, 16]: [f_start, f_width] x 4, then [t_start, t_width] x 4, as ww_spec_augment_draw writes them."""
    t_max = time_max(fraction, T) if t_max is None else int(t_max)
    rec = np.zeros((n, 16), dtype=np.int64)
    u = (word(seed, n, 0) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    on = u < np.float32(prob)
    for i in range(n_freq):
        w = int_in(word(seed, n, 1 + 2 * i), freq_max).astype(np.int64)
        rec[:, 2 * i] = int_in(word(seed, n, 2 + 2 * i), N_MELS - w)
        rec[:, 2 * i + 1] = w
    for i in range(n_time):
        w = int_in(word(seed, n, 9 + 2 * i), t_max).astype(np.int64)
        rec[:, 8 + 2 * i] = int_in(word(seed, n, 10 + 2 * i), T - w)
        rec[:, 8 + 2 * i + 1] = w
    rec[~on] = 0
    return rec.astype(np.int16)


def masks(records: np.ndarray, T: int) -> np.ndarray:
    """bool [n, 80, T]: True where a position is masked."""
    rec = np.asarray(records, dtype=np.int64)
    rows, cols = np.arange(N_MELS)[None, :], np.arange(T)[None, :]
    rm = np.zeros((rec.shape[0], N_MELS), dtype=bool)
    cm = np.zeros((rec.shape[0], T), dtype=bool)
    for i in range(4):
        f0, fw, t0, tw = rec[:, 2 * i, None], rec[:, 2 * i + 1, None], rec[:, 8 + 2 * i, None], rec[:, 9 + 2 * i, None]
        rm |= (rows >= f0) & (rows < f0 + fw)
        cm |= (cols >= t0) & (cols < t0 + tw)
    return rm[:, :, None] | cm[:, None, :]


def fills(mel: np.ndarray, fill) -> np.ndarray:
    """The exact fill value of every clip: float64 [n].  mel [n, 80, T] float32; fill "mean", "min" or a float."""
    x = np.asarray(mel, dtype=np.float32).reshape(mel.shape[0], -1)
    if fill == "mean":
        return x.astype(np.float64).mean(axis=1)
    if fill == "min":
        return np.fmin.reduce(x, axis=1).astype(np.float64)
    return np.full(x.shape[0], np.float32(fill), dtype=np.float64)


def apply(mel: np.ndarray, records: np.ndarray, fill="mean") -> np.ndarray:
    """The masked batch, float32 [n, 80, T]: the mean is the float64 mean rounded once to float32."""
    mel = np.asarray(mel, dtype=np.float32)
    out = mel.copy()
    m = masks(records, mel.shape[2])
    f = fills(mel, fill).astype(np.float32)
    out[m] = np.broadcast_to(f[:, None, None], mel.shape)[m]
    return out


def statistics(seed: int, n: int, T: int, **kw):
    """(share of clips masked at all, counts of frequency widths 0..freq_max among them, all masks in bounds)."""
    rec = draw_records(seed, n, T, **kw).astype(np.int64)
    on = word(seed, n, 0) >> np.uint64(40)
    on = on.astype(np.float32) * np.float32(2.0 ** -24) < np.float32(kw.get("prob", 0.8))
    fw = rec[on][:, 1:2 * kw.get("n_freq", 2):2].reshape(-1)
    counts = np.bincount(fw, minlength=kw.get("freq_max", 12) + 1)
    inb = bool(np.all(rec >= 0) and np.all(rec[:, 0:8:2] + rec[:, 1:8:2] <= N_MELS) and np.all(rec[:, 8:16:2] + rec[:, 9:16:2] <= T))
    return float(on.mean()), counts, inb
