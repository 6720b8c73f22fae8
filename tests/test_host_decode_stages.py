"""The float64 restatement of K0's stages (oracle/decode_oracle.py: mono_f64, resample_own_input, fma_chain_f32) against its definition,
and the teeth of the stage bounds tests/test_gpu_decode_stages.py asserts.  No GPU: the taps come from ww_resample_taps_host.

Bounds (u = 2^-24), all derived:
  resample, own input   |got[j] - y[j]| <= n[j] u A[j] + 2^-149
  definition            |y[j] - resample_poly(float64(x32))[j]| <= 6e-8 max(1, up) sum |x| over the output's frames (the float32 taps)
  conversion, 1 channel equality with float32(v scale);  C > 1 channels: <= C u mean|v|
"""
import numpy as np
import pytest
from scipy.signal import resample_poly

import k0_cases as k0
import wakeword_jupyterlab_amd as pkg
from oracle import decode_oracle as do

OLD_TOL = 5e-6                                                   # tests/test_gpu_decode.py's bound on a resampled row


def _tone(n, sr, seed):                                          # tests/test_gpu_decode.py's signal, as its files hold it (x 0.8, S16)
    t = np.arange(n) / sr
    x = 0.4 * np.sin(2 * np.pi * (180 + 37 * seed) * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t) + 0.05 * pkg.synth.normal(seed, n)
    return (np.clip(np.round(x * 0.8 * 32767), -32768, 32767) * 2.0 ** -15).astype(np.float32)


def _geometry(n_in, sr):
    """Per output: c (the tap index of frame 0), first and last frame of the chain -- from the upfirdn definition, for the mutations."""
    _, up, down, hl = k0.taps(sr)
    n_out, n_pre_pad, n_pre_remove, _ = do._poly_geometry(n_in, up, down, hl)
    c = (np.arange(n_out, dtype=np.int64) + n_pre_remove) * down - n_pre_pad
    i_lo = np.maximum(0, -((2 * hl - c) // up))
    i_hi = np.minimum(n_in - 1, np.where(c >= 0, c // up, -1))
    return c, i_lo, i_hi


@pytest.mark.parametrize("sr", k0.RATES)
def test_restatement_is_resample_poly_within_the_float32_taps(sr):
    t, up, down, hl = k0.taps(sr)
    worst = 0.0
    for n_in in k0.frame_counts(sr):
        _, x32 = do.mono_f64(k0.noise_s16(n_in, n_in), do.FMT_S16, 1)
        y, A, n = do.resample_own_input(x32, t, up, down, hl)
        ref = resample_poly(x32.astype(np.float64), up, down)
        assert y.shape == ref.shape == (k0.n_out_of(n_in, sr),) and n.min() >= 1 and n.max() <= (2 * hl + 1) // up + 1
        bound = do.TAP_TOL * max(1, up) * do.frames_abs_sum(x32, up, down, hl)
        assert (np.abs(y - ref) <= bound).all(), (sr, n_in, (np.abs(y - ref) / bound).max())
        worst = max(worst, (np.abs(y - ref) / bound).max())
        # the product count and the chain's frame range, derived twice (upfirdn on ones; the index formula of fma_chain_f32), agree
        c, i_lo, i_hi = _geometry(n_in, sr)
        assert np.array_equal(n, i_hi - i_lo + 1)
        if n_in <= 4001 * down // up + 2:                         # the bit-exact float32 chain obeys the stage bound it is the model for
            chain = do.fma_chain_f32(x32, t, up, down, hl)
            assert (np.abs(chain - y) <= do.stage_bound(A, n)).all()
    print(f"{sr} Hz: restatement vs resample_poly, worst share of the definition bound {worst:.3f}")


def test_fma_emulation_rounds_once():
    """fma_chain_f32's fmaf is x * h + y rounded ONCE.  up = down = 1, half_len = 1: y[0] = fmaf(x[1], h[0], fmaf(x[0], h[1], 0)).
    y = 2^30 + 128 (odd float32 mantissa), x h = 64 - 2^-40: the exact sum is just under the tie 2^30 + 192 and rounds to 2^30 + 128;
    float64 cannot hold it, rounds to the tie, and a second rounding to float32 (ties to even) would give 2^30 + 256."""
    x = np.array([2.0 ** 30 + 128, 8 * (1 + 2.0 ** -23)], np.float32)
    h = np.array([8 * (1 - 2.0 ** -23), 1.0, 0.0], np.float32)
    assert float(np.float32(float(x[0]) + float(x[1]) * float(h[0]))) == 2.0 ** 30 + 256        # the double rounding
    assert float(do.fma_chain_f32(x, h, 1, 1, 1)[0]) == 2.0 ** 30 + 128
    h[0] = 8 * (1 + 2.0 ** -23)                                   # x h = 64 + 2^-16 + 2^-40: above the tie, up
    assert float(do.fma_chain_f32(x, h, 1, 1, 1)[0]) == 2.0 ** 30 + 256


def _mutations(sr, x32):
    """name -> (mutated y, y, A, n) of the resampler mutations on the signal x32."""
    t, up, down, hl = k0.taps(sr)
    h = t.astype(np.float64)
    x = x32.astype(np.float64)
    y, A, n = do.resample_own_input(x32, t, up, down, hl)
    c, i_lo, i_hi = _geometry(len(x32), sr)
    out = {}
    xm = x32.copy(); xm[-1] = 0
    out["last frame dropped"] = do.resample_own_input(xm, t, up, down, hl)[0]
    xm = x32.copy(); xm[0] = 0
    out["first frame dropped"] = do.resample_own_input(xm, t, up, down, hl)[0]
    j = 2048                                                      # the first output of the second 2048-output block
    ii = np.arange(i_lo[j], i_hi[j] + 1)
    tt = c[j] - ii * up
    assert abs(np.sum(x[ii] * h[tt]) - y[j]) <= 1e-12
    ok = tt - up >= 0
    ym = y.copy(); ym[j] = np.sum(x[ii[ok]] * h[tt[ok] - up])
    out["tap index off by up at a seam output"] = ym
    # the chain's first product where the file's start does not cut the chain: the tap furthest from the centre.  At an integer ratio
    # (up = 1) that tap is the sinc's zero crossing, ~1e-19 -- dropping it changes nothing --, so the next one in is dropped there.
    t0 = c - i_lo * up
    lh = len(h)
    full = t0 >= lh - up
    k = np.where(np.abs(h[t0]) > 1e-9, 0, 1)
    out["outermost tap dropped"] = y - np.where(full, x[i_lo + k] * h[t0 - k * up], 0.0)
    return out, y, A, n


def test_teeth_of_the_stage_bounds():
    """Six faults applied to the float64 restatement on full-scale uniform noise (48 kHz and 44.1 kHz, 0.8 s): every one breaks the stage
    bound at one output or more.

    Record for test_gpu_decode.py's own `_tone` signal (same rates and length, whole row): NONE of the six stays inside its 5e-6 --
    last frame dropped 4e-2 (it carries the last outputs' centre taps), first frame dropped 4e-3, tap index off by `up` at the seam
    output 8e-3 .. 3e-2, outermost tap dropped 3e-4 (the signal's 5 % white noise is not in the stop band), 24-bit sign extension removed
    2.0, mean over C - 1 channels about the signal itself.  So what the old check misses is not these faults where it looks, but where it
    does not look: one length, one crop and one block layout per rate, eight rates -- a seam fault is seen only if the drawn crop holds
    the seam output -- and faults under 5e-6 (50 times the fma chain's own error).  The stage bound rejects all six on both signals."""
    inside = {}
    for sr in (48000, 44100):
        _, x_noise = do.mono_f64(k0.noise_s16(int(sr * 0.8), 5), do.FMT_S16, 1)
        for name, sig in (("noise", x_noise), ("tone", _tone(int(sr * 0.8), sr, 7))):
            muts, y, A, n = _mutations(sr, sig)
            for m, ym in muts.items():
                d = np.abs(ym - y)
                broke = (d > do.stage_bound(A, n)).sum()
                print(f"{sr} Hz {name:5s} {m:40s} max |dy| {d.max():.3e}  outputs over the stage bound {broke}")
                assert broke >= 1, (sr, name, m)
                if name == "tone":
                    inside[(sr, m)] = d.max() <= OLD_TOL
    assert not any(inside.values())                               # the docstring's record

    # conversion: the 24-bit sign extension removed; a channel mean over C - 1 channels
    rng = np.random.default_rng(3)
    codes = rng.integers(-(1 << 23), 1 << 23, size=3000)
    codes[:4] = [-(1 << 23), (1 << 23) - 1, -1, 0]
    m64, m32 = do.mono_f64(codes, do.FMT_S24, 1)
    assert np.array_equal(m32, (codes * 2.0 ** -23).astype(np.float32)) and np.array_equal(m64, m32.astype(np.float64))
    assert np.array_equal(do.codes_from_bytes(k0.to_bytes(codes, do.FMT_S24), do.FMT_S24), codes)
    unsigned = codes & 0xFFFFFF
    bad, _ = do.mono_f64(unsigned, do.FMT_S24, 1)
    assert (bad != m64).sum() == (codes < 0).sum() > 1000 and np.abs(bad - m64).max() == 2.0 > OLD_TOL
    for ch in (2, 3, 8):
        m64, m32 = do.mono_f64(codes[: 3000 // ch * ch], do.FMT_S24, ch)
        v = np.abs(codes[: 3000 // ch * ch].reshape(-1, ch) * 2.0 ** -23)
        bound = ch * do.U32 * v.mean(axis=1)
        assert (np.abs(m32 - m64) <= bound).all()                  # K0's sequential float32 mean is inside the conversion bound
        fewer = (codes[: 3000 // ch * ch].reshape(-1, ch)[:, : ch - 1] * 2.0 ** -23).mean(axis=1)
        assert (np.abs(fewer - m64) > bound).sum() > 900 // ch and np.abs(fewer - m64).max() > OLD_TOL


def test_conversion_scalings_and_extreme_codes():
    for fmt, lo, hi, scale in ((do.FMT_S16, -32768, 32767, 2.0 ** -15), (do.FMT_S24, -(1 << 23), (1 << 23) - 1, 2.0 ** -23),
                               (do.FMT_S32, -(1 << 31), (1 << 31) - 1, 2.0 ** -31)):
        m64, m32 = do.mono_f64(np.array([lo, hi, -1, 0]), fmt, 1)
        assert m64.tolist() == [-1.0, float(np.float32(hi * scale)), -scale, 0.0] and np.array_equal(m32, m64.astype(np.float32))
    m64, _ = do.mono_f64(np.array([0, 255, 127, 128]), do.FMT_U8, 1)
    assert m64.tolist() == [-1.0, 127 / 128, -1 / 128, 0.0]
    m64, m32 = do.mono_f64(np.array([1 / 3, -1 + 2.0 ** -30]), do.FMT_F64, 1)
    assert m32.tolist() == [float(np.float32(1 / 3)), -1.0]
    # the byte round trip of every format
    for fmt, codes in ((do.FMT_S16, [-32768, 32767, -1, 0]), (do.FMT_U8, [0, 255, 127, 128]), (do.FMT_S32, [-(1 << 31), (1 << 31) - 1, -1, 0]),
                       (do.FMT_F32, [-1.0, 1.0, 0.25, 0.0]), (do.FMT_F64, [-1.0, 1 / 3, 0.25, 0.0])):
        assert np.array_equal(do.codes_from_bytes(k0.to_bytes(np.array(codes), fmt), fmt), np.array(codes))
