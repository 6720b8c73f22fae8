"""CPU restatement of the load -> normalise -> crop/pad front of process_audio_file (TEST INFRASTRUCTURE ONLY).

Follows /root/reference/wakeword_training_script.py:65-83,125-133:
    librosa.load(path, sr=16000)  = soundfile decode to float32 (ints / 2^(bits-1)), librosa.to_mono (channel mean),
                                    resample to 16 kHz
    normalize_audio               = x / max|x| over the whole file
    pad_or_truncate               = random crop (start drawn by the caller) or right zero-pad to 16000

PARITY UNPINNED for the resampler: librosa 0.10's default is soxr_hq (a third-party library, not installed).  This
restatement -- and the GPU kernel -- use scipy.signal.resample_poly's Kaiser-windowed-sinc polyphase design instead;
files already at 16 kHz are decoded exactly.
"""
from math import gcd

import numpy as np
from scipy.signal import resample_poly, upfirdn

SAMPLE_RATE = 16000
CLIP = 16000


def decode(samples: np.ndarray, sample_rate: int) -> np.ndarray:
    """samples: float [n_frames, channels] already scaled to [-1, 1) as soundfile does -> mono 16 kHz float64."""
    x = np.asarray(samples, dtype=np.float32)
    mono = x.mean(axis=1, dtype=np.float32) if x.shape[1] > 1 else x[:, 0]
    if sample_rate == SAMPLE_RATE:
        return mono.astype(np.float64)
    g = gcd(SAMPLE_RATE, int(sample_rate))
    return resample_poly(mono.astype(np.float64), SAMPLE_RATE // g, int(sample_rate) // g)


def load_normalise_crop(samples, sample_rate, crop_start=0, normalize=True) -> np.ndarray:
    y = decode(samples, sample_rate)
    if normalize and len(y):
        with np.errstate(invalid="ignore", divide="ignore"):
            y = y / np.max(np.abs(y))
    y = y[crop_start:crop_start + CLIP]
    return np.pad(y, (0, CLIP - len(y))).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# K0 stage by stage, each stage against float64 ON ITS OWN INPUT (tests/test_host_decode_stages.py, tests/test_gpu_decode_stages.py)
# ---------------------------------------------------------------------------------------------
U32 = 2.0 ** -24                                                 # float32 unit roundoff
TAP_TOL = 6e-8                                                   # tests/test_host_native.py's bound on a float32 tap, times max(1, up)
FMT_S16, FMT_S24, FMT_S32, FMT_F32, FMT_U8, FMT_F64 = 1, 2, 3, 4, 5, 6     # WW_FMT_* (include/wakeword_amd.h)
SAMPLE_BYTES = {FMT_S16: 2, FMT_S24: 3, FMT_S32: 4, FMT_F32: 4, FMT_U8: 1, FMT_F64: 8}


def codes_from_bytes(buf, fmt) -> np.ndarray:
    """Little-endian sample bytes as a WAV data chunk holds them -> integer codes (int64) or float samples (float32 / float64)."""
    b = np.frombuffer(bytes(buf), dtype=np.uint8)
    if fmt == FMT_S24:
        t = b.reshape(-1, 3).astype(np.int64)
        v = t[:, 0] + 256 * t[:, 1] + 65536 * t[:, 2]
        return v - (v >= 1 << 23) * (1 << 24)                    # two's complement of 24 bits
    dt = {FMT_S16: "<i2", FMT_S32: "<i4", FMT_U8: "u1", FMT_F32: "<f4", FMT_F64: "<f8"}[fmt]
    v = b.view(dt)
    return v.astype(np.int64) if fmt in (FMT_S16, FMT_S32, FMT_U8) else v.copy()


def mono_f64(raw_samples, fmt, channels):
    """Interleaved codes / float samples -> (float64 channel mean, the float32 mono K0 forms).

    A sample's value is soundfile's float32: float32(code * 2^-15), (code - 128) / 128, float32(code * 2^-23), float32(code * 2^-31),
    float32(sample) -- one rounding at most (S32 codes above 2^24, F64 samples), which belongs to the conversion's definition.  The float64
    mean is taken over those values.  K0's mono is their SEQUENTIAL float32 sum from 0.f over the channels in order, divided by
    float32(channels) when channels > 1 (sample_mono in csrc/ww_decode.hip; checked there: `s += v` in a loop, no tree, no fma)."""
    v = np.asarray(raw_samples)
    if fmt in (FMT_F32, FMT_F64):
        with np.errstate(over="ignore"):
            v32 = v.astype(np.float32)
    else:
        v = v.astype(np.float64)
        scale = {FMT_S16: 2.0 ** -15, FMT_S24: 2.0 ** -23, FMT_S32: 2.0 ** -31, FMT_U8: 2.0 ** -7}[fmt]
        v32 = ((v - 128.0 if fmt == FMT_U8 else v) * scale).astype(np.float32)
    v32 = v32.reshape(-1, channels)
    m64 = v32.astype(np.float64).mean(axis=1)
    if channels == 1:
        return m64, v32[:, 0].copy()
    s = np.zeros(len(v32), np.float32)
    for c in range(channels):
        s = (s + v32[:, c]).astype(np.float32)
    return m64, (s / np.float32(channels)).astype(np.float32)


def _poly_geometry(n_in, up, down, half_len):
    """resample_poly's bookkeeping around upfirdn: zeros in front of h so that the centre tap falls on an output, outputs removed in front,
    zeros behind h so that upfirdn yields n_out outputs after them (scipy/signal/_signaltools.py, resample_poly)."""
    n_out = n_in * up // down + bool(n_in * up % down)
    n_pre_pad = down - half_len % down
    n_pre_remove = (half_len + n_pre_pad) // down
    lh = 2 * half_len + 1
    n_post_pad = 0
    while ((n_in - 1) * up + lh + n_pre_pad + n_post_pad - 1) // down + 1 < n_out + n_pre_remove:     # upfirdn's output length
        n_post_pad += 1
    return n_out, n_pre_pad, n_pre_remove, n_post_pad


def resample_own_input(x32, taps32, up, down, half_len):
    """The resampler stage on K0's own float32 mono and its own float32 taps, in float64: y[j] = sum_i x[i] h[c_j - i up].
    Returns (y, A, n): A[j] = sum_i |x[i]| |h[c_j - i up]|, n[j] = the number of products of output j (frames inside the file whose tap is
    inside the filter; a tap that happens to be 0.0 counts).  The index ranges are scipy.signal.upfirdn's, sliced as resample_poly slices."""
    x = np.asarray(x32, dtype=np.float64)
    h = np.asarray(taps32, dtype=np.float64)
    assert h.shape == (2 * half_len + 1,)
    if len(x) == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0, np.int64)
    n_out, n_pre_pad, n_pre_remove, n_post_pad = _poly_geometry(len(x), up, down, half_len)
    keep = slice(n_pre_remove, n_pre_remove + n_out)

    def run(hh, xx):
        full = upfirdn(np.concatenate([np.zeros(n_pre_pad), hh, np.zeros(n_post_pad)]), xx, up, down)
        assert len(full) >= n_pre_remove + n_out
        return full[keep]
    n = np.rint(run(np.ones_like(h), np.ones_like(x))).astype(np.int64)
    return run(h, x), run(np.abs(h), np.abs(x)), n


def frames_abs_sum(x32, up, down, half_len):
    """sum of |x[i]| over the frames of each output (the definition bound's weight)."""
    x = np.abs(np.asarray(x32, dtype=np.float64))
    _, a, _ = resample_own_input(x, np.ones(2 * half_len + 1), up, down, half_len)
    return a


def stage_bound(A, n):
    """|got[j] - y[j]| <= n[j] u A[j] + 2^-149: one rounding per fused multiply-add of the chain (the standard gamma_n bound to first
    order), and the smallest float32 for a chain that underflows."""
    return n * U32 * A + 2.0 ** -149


def fma_chain_f32(x32, taps32, up, down, half_len):
    """The direct form in float32, bit for bit: y = 0.f; for the output's frames i ascending: y = fmaf(x[i], h[c - i up], y).
    Output j' of upfirdn(hp, x, up, down) is sum_i x[i] hp[j' down - i up]; hp = h behind n_pre_pad zeros, j' = j + n_pre_remove.
    fmaf is emulated exactly: the product of two float32 is exact in float64, TwoSum gives the float64 sum's error, and where the float64
    sum sits exactly half way between two float32 the error's sign decides the rounding."""
    x32 = np.asarray(x32, dtype=np.float32)
    h = np.asarray(taps32, dtype=np.float64)
    lh = 2 * half_len + 1
    if len(x32) == 0:
        return np.zeros(0, np.float32)
    n_out, n_pre_pad, n_pre_remove, _ = _poly_geometry(len(x32), up, down, half_len)
    c = (np.arange(n_out, dtype=np.int64) + n_pre_remove) * down - n_pre_pad     # index into h of frame 0's tap
    i_lo = np.maximum(0, -((lh - 1 - c) // up))                   # smallest i with c - i up <= lh - 1
    i_hi = np.minimum(len(x32) - 1, np.where(c >= 0, c // up, -1))
    x = x32.astype(np.float64)
    y = np.zeros(n_out, np.float32)
    for k in range(int((i_hi - i_lo).max()) + 1 if n_out else 0):
        i = i_lo + k
        live = i <= i_hi
        ii = np.where(live, i, 0)
        p = x[ii] * h[np.where(live, c - ii * up, 0)]
        y64 = y.astype(np.float64)
        s = p + y64
        bb = s - p
        e = (p - (s - bb)) + (y64 - bb)                           # p + y64 == s + e exactly
        with np.errstate(over="ignore"):
            r = s.astype(np.float32)
            rd = r.astype(np.float64)
            other = np.where(rd > s, np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))).astype(np.float64)
        tie = (np.abs(rd - s) == np.abs(other - s)) & (e != 0) & np.isfinite(rd) & np.isfinite(other)
        toward_other = tie & (np.sign(e) == np.sign(other - rd))
        r = np.where(toward_other, other, rd)                     # (else the cast's choice stands)
        y = np.where(live, r, y64).astype(np.float32)
    return y
