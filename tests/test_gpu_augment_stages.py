"""Each stage of the augmentation chain (csrc/ww_augment.hip: roll -> stft_pv -> istft -> resample) against float64 ON ITS OWN INPUT.

The end-to-end bound of tests/test_gpu_augment*.py (3e-3 of the peak, 1e-3 of the rms) is set by librosa's float32 phase accumulator
(tests/test_oracle_augment.py::test_phase_vocoder_conditioning_sets_the_gpu_tolerance) and is about a thousand times wider than the
rounding error of the stages that are not chaotic.  Here ops.augment_stages reads the chain's intermediates from the workspace of the call
(ww_augment_workspace_layout) and every stage is compared with oracle/augment_oracle.py's float64 entry points fed what the kernel itself
was fed, as tests/test_gpu_train.py replays the reference with the kernel's own sign images:

  (a) roll        the work buffer the STFT reads == np.roll bit for bit, its row padding zero
  (b) magnitudes  |S[t, k]| against (1 - alpha) |D[i0, k]| + alpha |D[i0 + 1, k]|, D = float64 STFT of the rolled clip.  Allowance, as a
                  fraction of max |D|: 4 x the error of a float32 restatement on the CPU (scipy's float32 rfft of the float32 windowed
                  frame, float32 abs and interpolation), measured on the same clip, + 2 * 2^-24 (the kernel's FFT is another
                  factorisation, its |c| a 1-ulp square root)
  (c) phase       one accumulator step: angle(S[t+1, k] conj S[t, k]) against (phi_k + wrapped dphase[t, k]) mod 2 pi.  Allowance per
                  (t, k): ulp32(|acc| + 8 pi) (acc = the oracle's float64 accumulator at the step; the float32 one is rounded before and
                  after, and may sit a few turns away) + 2 e_D / rho (two atan2 of columns whose error is e_D max |D|, e_D = 4 x the
                  float32 restatement's figure of (b), on bins with min(|c0|, |c1|) >= rho max |D|, rho = 1e-3) + 4e-6 (v_sin / v_cos 1e-6,
                  the polynomial atan2 1.2e-7, twice each).  Left out: bins under rho, steps whose dphase / 2 pi is within
                  2 e_D / rho / 2 pi of a half-integer (either wrap is right), the last step (it has no successor).  On the
                  synth.make_clips clips at most 20 % of the (t, k) pairs are left out and every bin is checked at least once, asserted
                  from the oracle alone.  angle(S[0, k]) against angle(D[0, k]): e_D / rho + 2e-6 (one column, one atan2, one v_sin / v_cos)
  (d) istft       float64 istft of the kernel's own S against Y (pitch) / the cropped, zero-padded stage (stretch).  Allowance as a
                  fraction of max |y|: 4 x the error of the oracle's float32-accumulating istft on the same S + 2 * 2^-24, measured here
  (e) resampler   float64 resample of the kernel's own Y.  Derived bound per output: (taps + 6) 2^-24 sum_i |w_i y_i| + 2^-24 |out|
                  (taps = the longer wing's fma chain; + float32 table entry, the interpolation fma, the two wings added, the ratio gain
                  and its rounding, the final store): no measured constant
  (f) teeth       on the CPU: faults of the kind the end-to-end bound hides, applied to the oracle, are rejected by (b)-(e)'s comparison
                  functions, while the old bound accepts a nearest-row table and a last tap dropped on full-length wings
  (g) compose     pitch-only output fed to a stretch-only call == the combined call, bit for bit

Measured figures: every check prints its float32-restatement error, the kernel's error and the allowance; with WW_AUG_STAGE_JSON=path the
module writes them to that file when it is done (scripts/aug_stage_errors.py -> profiles/aug_stage_errors.json)."""
import json
import os

import numpy as np
import pytest
import scipy.fft

import wakeword_jupyterlab_amd as pkg
from oracle import augment_oracle as ao

U = 2.0 ** -24
RHO = 1e-3
NS = (4000, 5001, 12345, 16000, 16383)
STRETCH_RATES = (32 / 46, 0.7, 0.91, 1.0, 1.3)
PITCH_STEPS = (-3.0, -1.3, 0.5, 3.0)
PITCH_RATE_EXACT = 0.8125                    # ratio * 512 = 416 exactly: index_step must not come out as 415
PITCH_RATE_NEAR = 0.9375                     # 16000 / (16000 / rate) * 512 = 479.99999999999994: index_step is 479, as resampy's int()
KINDS = ("tonal", "noise", "speech", "half_silent", "zero")
OFF = {"shift": 0, "n_steps": None, "rate": None, "crop": 0, "sigma": 0.0, "seed": 0}
FIGURES = []


@pytest.fixture(scope="module", autouse=True)
def _figures_file():
    yield
    path = os.environ.get("WW_AUG_STAGE_JSON")
    if path and FIGURES:
        with open(path, "w") as f:
            json.dump(FIGURES, f, indent=1)


def _clip(kind, n):
    """tonal / noise: synth.make_clips' two kinds (clips 3 and 4).  speech: make_clips has no such kind -- harmonics of a gliding pitch
    under a 4 Hz syllable envelope over weak noise, from the same generator.  half_silent: the noise clip, zero from n // 2 on."""
    if kind == "tonal":
        x = pkg.synth.make_clips(3, 1, n=n)[0]
    elif kind in ("noise", "half_silent"):
        x = pkg.synth.make_clips(4, 1, n=n)[0].copy()
        if kind == "half_silent":
            x[n // 2:] = 0.0
    elif kind == "speech":
        t = np.arange(n) / 16000.0
        f0 = 120.0 + 40.0 * np.sin(2 * np.pi * 1.5 * t)
        ph = 2 * np.pi * np.cumsum(f0) / 16000.0
        voiced = sum(np.sin(h * ph) / h for h in range(1, 12))
        env = 0.05 + np.clip(np.sin(2 * np.pi * 4.0 * t), 0.0, None) ** 2
        x = (0.25 * env * voiced + 0.02 * pkg.synth.normal(77, n)).astype(np.float32)
    else:
        return np.zeros(n, np.float32)
    return (x / np.abs(x).max()).astype(np.float32)


def _ulp32(a):
    a = np.maximum(np.asarray(a, dtype=np.float64), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


def _old_check(got, want, max_rel=3e-3, rms_rel=1e-3):
    """tests/test_gpu_augment.py's end-to-end comparison."""
    err = got.astype(np.float64) - want.astype(np.float64)
    peak, rms = np.abs(want).max(), np.sqrt((want.astype(np.float64) ** 2).mean())
    assert np.abs(err).max() <= max_rel * peak, (np.abs(err).max() / peak)
    assert np.sqrt((err ** 2).mean()) <= rms_rel * rms, (np.sqrt((err ** 2).mean()) / rms)


# ---- the comparison functions: numpy in, figures out, AssertionError on a miss ------------------------------------------------------
def _mags32(y, pv):
    """(b)'s float32 restatement: float32 window product, scipy's float32 rfft, float32 abs and interpolation."""
    yp = np.pad(np.asarray(y, np.float32), (ao.N_FFT // 2, ao.N_FFT // 2))
    w = ao.hann().astype(np.float32)
    T = 1 + len(y) // ao.HOP
    m = np.zeros((ao.N_FFT // 2 + 1, T + 2), np.float32)
    for t in range(T):
        c = scipy.fft.rfft(w * yp[t * ao.HOP:t * ao.HOP + ao.N_FFT])
        assert c.dtype == np.complex64
        m[:, t] = np.abs(c)
    i0, alpha = pv["i0"], pv["alpha"]
    return (1.0 - alpha).astype(np.float32) * m[:, i0] + alpha.astype(np.float32) * m[:, i0 + 1]


def check_magnitudes(S, rolled, rate, label=""):
    """(b).  S complex [steps, 1025] (the kernel's), rolled float32 [n] -> figures; e_D = 4 x the float32 restatement's error."""
    D = ao.stft64(rolled)
    pv = ao.pv_steps(D, rate)
    assert S.shape == (len(pv["i0"]), D.shape[0]), (S.shape, len(pv["i0"]))
    got = np.abs(np.asarray(S, np.complex128)).T
    dmax = np.abs(D).max()
    if dmax == 0.0:
        assert np.all(got == 0.0), "a zero clip must give S == 0 exactly"
        return {"stage": "magnitudes", "case": label, "f32": 0.0, "kernel": 0.0, "allow": 0.0, "e_D": 0.0}, D, pv
    silent = (pv["c0"] == 0.0) & (pv["c1"] == 0.0)               # both columns lie in exact silence
    assert np.all(got[silent] == 0.0), "steps whose columns are silent must give S == 0 exactly"
    f32 = float(np.abs(_mags32(rolled, pv).astype(np.float64) - pv["mag"]).max() / dmax)
    err = float(np.abs(got - pv["mag"]).max() / dmax)
    allow = 4.0 * f32 + 2.0 * U
    fig = {"stage": "magnitudes", "case": label, "f32": f32, "kernel": err, "allow": allow, "e_D": 4.0 * f32}
    print(f"(b) {label}: float32 restatement {f32:.3e}, kernel {err:.3e}, allowance {allow:.3e} of max|D|")
    assert err <= allow, fig
    return fig, D, pv


def phase_mask(D, pv, e_D):
    """(c)'s kept (k, t) pairs, from the oracle alone -> (keep [1025, steps], left-out share, bins never checked)."""
    dmax = np.abs(D).max()
    n_steps = len(pv["i0"])
    keep = np.minimum(pv["c0"], pv["c1"]) >= RHO * dmax
    if dmax == 0.0:
        keep[:] = False
    frac = pv["turns"] - np.floor(pv["turns"])
    keep &= np.abs(frac - 0.5) > 2.0 * e_D / RHO / (2.0 * np.pi)
    keep[:, n_steps - 1] = False                                  # no successor
    keep[:, :-1] &= pv["mag"][:, 1:] > 0.0                        # the successor's column must have an angle at all (exact silence has none)
    return keep, 1.0 - keep.mean(), int((~keep.any(axis=1)).sum())


def check_phase(S, D, pv, e_D, label="", require_share=True):
    """(c).  One accumulator step at a time."""
    S = np.asarray(S, np.complex128).T                            # [1025, steps]
    keep, left_out, unchecked = phase_mask(D, pv, e_D)
    if require_share:
        assert left_out <= 0.20 and unchecked == 0, (label, left_out, unchecked)
    two_pi = 2.0 * np.pi
    meas = np.angle(S[:, 1:] * np.conj(S[:, :-1]))
    diff = meas - pv["advance"][:, :-1]
    diff = np.abs(diff - two_pi * np.round(diff / two_pi))
    acc = np.abs(pv["acc"])
    A = np.maximum(acc[:, :-1], acc[:, 1:]) + 8.0 * np.pi
    tol = _ulp32(A) + 2.0 * e_D / RHO + 4e-6
    k = keep[:, :-1]
    worst = float((diff[k] / tol[k]).max()) if k.any() else 0.0
    # the first column: acc = atan2(D[:, 0])
    k0 = np.abs(D[:, 0]) >= RHO * max(np.abs(D).max(), 1e-300)
    d0 = np.angle(S[:, 0]) - np.angle(D[:, 0])
    d0 = np.abs(d0 - two_pi * np.round(d0 / two_pi))
    tol0 = e_D / RHO + 2e-6
    worst0 = float((d0[k0] / tol0).max()) if k0.any() else 0.0
    fig = {"stage": "phase", "case": label, "share_asserted": bool(require_share), "left_out": float(left_out), "bins_unchecked": unchecked, "pairs_checked": int(k.sum()),
           "kernel_over_allow": worst, "max_err_rad": float(diff[k].max()) if k.any() else 0.0, "first_column_over_allow": worst0,
           "e_D": e_D}
    print(f"(c) {label}: {k.sum()} pairs, left out {100 * left_out:.1f} %, worst err / allowance {worst:.3f} (max {fig['max_err_rad']:.3e} rad), "
          f"first column {worst0:.3f}")
    assert worst <= 1.0 and worst0 <= 1.0, fig
    return fig


def check_istft(S, got, length, crop, label=""):
    """(d).  S complex [steps, 1025] (the kernel's own), got float32 [m] = y[crop : crop + m], zero past `length`."""
    St = np.asarray(S, np.complex128).T
    want = ao.istft64(St, length)
    f32 = ao.istft(St, length).astype(np.float64)
    peak = np.abs(want).max()
    e32 = float(np.abs(f32 - want).max() / peak) if peak > 0 else 0.0
    m = len(got)
    ref = np.zeros(m)
    seg = want[crop:crop + m]
    ref[:len(seg)] = seg
    assert np.isfinite(got).all()
    if length - crop < m:
        assert np.all(got[length - crop:] == 0.0), "samples at and past the stretched length must be zero"
    err = float(np.abs(got.astype(np.float64) - ref).max() / peak) if peak > 0 else float(np.abs(got).max())
    allow = 4.0 * e32 + 2.0 * U if peak > 0 else 0.0
    fig = {"stage": "istft", "case": label, "f32": e32, "kernel": err, "allow": allow}
    print(f"(d) {label}: float32 istft {e32:.3e}, kernel {err:.3e}, allowance {allow:.3e} of max|y|")
    assert err <= allow, fig
    return fig


def check_resample(Y, got, ratio, p_res, label="", terms=None):
    """(e).  Y float32 [p_len] (the kernel's own), got float32 [n] -> figures; the edge and tail outputs must be present."""
    n, p_len = len(got), len(Y)
    y, absum, i_max, k_max = terms if terms is not None else ao.resample_terms(Y, ratio)
    assert len(y) == p_res, (len(y), p_res)
    m = min(n, p_res)
    want, bound = np.zeros(n), np.zeros(n)
    want[:m] = y[:m]
    taps = np.maximum(i_max, k_max)[:m]
    bound[:m] = (taps + 6) * U * absum[:m] + U * np.abs(got[:m].astype(np.float64))
    assert np.isfinite(got).all()
    dead = np.ones(n, bool)
    dead[:m] = i_max[:m] < 0                                       # int(t / ratio) >= p_len
    assert np.all(got[dead] == 0.0), "outputs past the resampled length must be zero"
    live = ~dead
    tails = {r: int(((i_max[:m] % 4 == r) & live[:m]).sum()) + int(((k_max[:m] % 4 == r) & live[:m]).sum()) for r in (1, 2, 3)}
    assert all(v > 0 for v in tails.values()) and live[:200].all() and live[m - 200:m].sum() >= 190, (label, tails)
    err = np.abs(got.astype(np.float64) - want)
    peak = np.abs(want).max()
    ratio_to_bound = float((err[live] / np.maximum(bound[live], 1e-300)).max()) if peak > 0 else 0.0
    fig = {"stage": "resample", "case": label, "kernel_over_bound": ratio_to_bound, "kernel": float(err.max() / peak) if peak > 0 else float(err.max()),
           "bound_of_peak": float(bound.max() / peak) if peak > 0 else 0.0, "tails": tails,
           "edge_over_bound": float(max((err[:200] / np.maximum(bound[:200], 1e-300)).max(),
                                        (err[m - 200:m] / np.maximum(bound[m - 200:m], 1e-300)).max())) if peak > 0 else 0.0}
    print(f"(e) {label}: kernel err {fig['kernel']:.3e} of the peak, bound {fig['bound_of_peak']:.3e}, worst err / bound {ratio_to_bound:.3f} "
          f"(first / last 200 outputs {fig['edge_over_bound']:.3f}), tails {tails}")
    if peak > 0:
        assert np.all(err <= bound), fig
    else:
        assert np.all(got == 0.0)
    return fig


# ---- (f) teeth, and the oracle's float64 entry points: CPU only ------------------------------------------------------------------------
def test_float64_entry_points_agree_with_the_pinned_oracle():
    y = _clip("tonal", 5001)
    D, D64 = ao.stft(y), ao.stft64(y)
    assert D64.dtype == np.complex128 and np.abs(D - D64).max() <= 2.0 ** -23 * np.abs(D64).max()
    S = ao.phase_vocoder(D, 0.8)
    pv = ao.pv_steps(D, 0.8)
    assert S.shape[1] == len(pv["i0"]) == 13 and np.abs(np.abs(S) - pv["mag"]).max() <= 4 * U * np.abs(D).max()
    # the float64 accumulator follows librosa's float32 one to the float32 rounding of its steps
    acc32 = np.angle(S[:, -1].astype(np.complex128))
    d = acc32 - pv["acc"][:, -1]
    d = np.abs(d - 2 * np.pi * np.round(d / (2 * np.pi)))
    strong = np.abs(S[:, -1]) > 1e-2 * np.abs(D).max()
    assert np.median(d[strong]) < 0.05
    z = ao.istft(S, 6251)
    assert np.abs(z - ao.istft64(S, 6251)).max() <= 8 * U * np.abs(z).max()
    for ratio in (0.84, 1.19):
        r, absum, i_max, k_max = ao.resample_terms(y, ratio)
        assert np.array_equal(r.astype(np.float32), ao.resample(y, ratio))
        full = 76 if ratio < 1 else 64                          # (32769 - offset) // index_step at offset 0
        assert np.all(absum >= np.abs(r) - 1e-12) and i_max.max() == full and k_max.max() in (full - 1, full)
        assert i_max[0] == 1 and k_max[len(r) - 1] <= 1


def _f32_resample(Y, ratio, n, weights=None):
    z = ao.resample_terms(Y, ratio, weights)[0].astype(np.float32)
    out = np.zeros(n, np.float32)
    out[:min(n, len(z))] = z[:n]
    return out


def _istft_dropping(S, length, drop_seg):
    """ao.istft64 with hop segment `drop_seg` of the padded signal summed without its earliest frame (three frames instead of four)."""
    S = np.asarray(S, np.complex128)
    n_frames = min(S.shape[1], -(-(length + ao.N_FFT) // ao.HOP))
    w = ao.hann()
    full, wss = np.zeros(ao.N_FFT + ao.HOP * (n_frames - 1)), np.zeros(ao.N_FFT + ao.HOP * (n_frames - 1))
    for t in range(n_frames):
        fr, ww = w * np.fft.irfft(S[:, t], n=ao.N_FFT), w * w
        if t == drop_seg - 3:
            fr[3 * ao.HOP:], ww = 0.0, np.concatenate([ww[:3 * ao.HOP], np.zeros(ao.HOP)])
        full[t * ao.HOP:t * ao.HOP + ao.N_FFT] += fr
        wss[t * ao.HOP:t * ao.HOP + ao.N_FFT] += ww
    y = np.zeros(length)
    seg, ws = full[ao.N_FFT // 2:ao.N_FFT // 2 + length], wss[ao.N_FFT // 2:ao.N_FFT // 2 + length]
    y[:len(seg)] = np.where(ws > np.finfo(np.float32).tiny, seg / np.maximum(ws, 1e-300), seg)
    return y


@pytest.mark.parametrize("n", (4000, 16000))
@pytest.mark.parametrize("kind", ("tonal", "noise", "half_silent"))
def test_teeth_the_stage_checks_reject_what_the_end_to_end_bound_accepts(n, kind):
    x = _clip(kind, n)
    rate = ao.pitch_rate(3.0)                                     # ratio < 1, index_step 430
    # -- (b), (c): a float32 restatement of the vocoder passes; alpha / the advance of the next step do not
    D = ao.stft64(x)
    pv = ao.pv_steps(D, rate)
    S = (pv["mag"] * np.exp(1j * pv["acc"])).astype(np.complex64).T
    fig, _, _ = check_magnitudes(S, x, rate, "teeth")
    check_phase(S, D, pv, fig["e_D"], "teeth", require_share=kind != "half_silent")
    nxt = np.append(pv["alpha"][1:], pv["alpha"][0])
    bad = (((1.0 - nxt) * pv["c0"] + nxt * pv["c1"]) * np.exp(1j * pv["acc"])).astype(np.complex64).T
    with pytest.raises(AssertionError):
        check_magnitudes(bad, x, rate, "alpha of the next step")
    adv = np.concatenate([pv["advance"][:, 1:], pv["advance"][:, :1]], axis=1)
    acc = np.angle(D[:, :1]) + np.concatenate([np.zeros((1025, 1)), np.cumsum(adv, axis=1)[:, :-1]], axis=1)
    with pytest.raises(AssertionError):
        check_phase((pv["mag"] * np.exp(1j * acc)).astype(np.complex64).T, D, pv, fig["e_D"], "advance of the next step", require_share=False)
    # -- (d): crop + 1, and the first four-frame hop segment summed from three frames
    s_rate = 0.7
    length = int(round(n / s_rate))
    crop = length - n
    Ss = ao.phase_vocoder(ao.stft(x), s_rate).T
    y64 = ao.istft64(Ss.T, length)
    check_istft(Ss, y64[crop:crop + n].astype(np.float32), length, crop, "teeth")
    with pytest.raises(AssertionError):
        check_istft(Ss, y64[crop + 1:crop + 1 + n].astype(np.float32), length, crop, "crop + 1")
    with pytest.raises(AssertionError):
        check_istft(Ss, _istft_dropping(Ss.T, length, 3)[:n].astype(np.float32), length, 0, "three frames")
    last_seg = (ao.N_FFT // 2 + length - 1) // ao.HOP
    if kind != "half_silent":                                      # (its last segments are silent: nothing to drop)
        with pytest.raises(AssertionError):
            check_istft(Ss, _istft_dropping(Ss.T, length, last_seg)[crop:crop + n].astype(np.float32), length, crop, "three frames, last")
    # -- (e): the resampler's table lookup and tails
    for n_steps in (3.0, -3.0):
        rate = ao.pitch_rate(n_steps)
        ratio = 16000.0 / (16000.0 / rate)
        Y = ao.time_stretch(x, rate)
        p_res = int(np.ceil(len(Y) * ratio))
        terms = ao.resample_terms(Y, ratio)
        want = _f32_resample(Y, ratio, n)
        check_resample(Y, want, ratio, p_res, "teeth", terms)
        nearest = _f32_resample(Y, ratio, n, lambda win, delta, idx, eta: win[idx])

        def drop_last(full_only, wing=[0]):                       # the left wing's last tap
            def f(win, delta, idx, eta):
                w = win[idx] + eta * delta[idx]
                wing[0] ^= 1
                if wing[0] == 1 and len(idx) and (not full_only or len(idx) == (len(win) - idx[0]) // (idx[1] - idx[0] if len(idx) > 1 else 1)):
                    w[-1] = 0.0
                return w
            return f
        dropped = _f32_resample(Y, ratio, n, drop_last(False, [0]))
        dropped_full = _f32_resample(Y, ratio, n, drop_last(True, [0]))
        upper = _f32_resample(Y, ratio, n, lambda win, delta, idx, eta: win[idx] + (1.0 - eta) * delta[idx])
        for name, bad in (("nearest row", nearest), ("last tap dropped", dropped), ("eta of the other neighbour", upper)):
            with pytest.raises(AssertionError):
                check_resample(Y, bad, ratio, p_res, name, terms)
        # A last tap dropped on full-length wings only: the tap weighs ~1e-8 of the sum, under the float32 rounding of any clip that is loud
        # throughout -- no comparison of values can see it there.  The half-silent clip shows it: where the stretched clip is exactly zero
        # and only a wing's last tap still reaches the sound, that tap IS the sum (which is why the GPU cases carry this clip).
        if kind == "half_silent":
            with pytest.raises(AssertionError):
                check_resample(Y, dropped_full, ratio, p_res, "last tap dropped on full wings", terms)
        # what the end-to-end bound makes of them: it accepts the full-wing drop on every clip; the nearest-row table passes its peak
        # criterion (2e-3 of 3e-3) and is caught only by the rms one, at 1.9e-3 .. 2.1e-3 of the rms against 1e-3 (a factor of two,
        # where the derived bound is exceeded 400-fold)
        _old_check(dropped_full, want)
        err = np.abs(nearest.astype(np.float64) - want)
        print(f"nearest-row table under the end-to-end bound: max {err.max() / np.abs(want).max():.2e} of the peak, "
              f"rms {np.sqrt((err ** 2).mean() / (want.astype(np.float64) ** 2).mean()):.2e} of the rms")
        assert err.max() <= 3e-3 * np.abs(want).max()


def test_phase_mask_keeps_enough_of_every_make_clips_clip():
    """(c)'s condition from the oracle alone: clips 0..11 at the shortest and the 1 s length, every rate of the GPU cases."""
    for n in (4000, 16000):
        for i in range(12):
            x = pkg.synth.make_clips(i, 1, n=n)[0]
            D = ao.stft64(x)
            for rate in STRETCH_RATES + tuple(ao.pitch_rate(s) for s in PITCH_STEPS) + (PITCH_RATE_EXACT, PITCH_RATE_NEAR):
                pv = ao.pv_steps(D, rate)
                e_D = 4.0 * float(np.abs(_mags32(x, pv).astype(np.float64) - pv["mag"]).max() / np.abs(D).max())
                _, left_out, unchecked = phase_mask(D, pv, e_D)
                assert left_out <= 0.20 and unchecked == 0, (n, i, rate, left_out, unchecked)


# ---- the GPU stages -------------------------------------------------------------------------------------------------------------------
def _stages(x, plans, poison=True):
    import torch
    from wakeword_jupyterlab_amd import ops
    st = ops.augment_stages(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.device("cuda", 0)), plans, poison=poison)
    return {k: ([t.cpu().numpy() for t in v] if isinstance(v, list) else v if isinstance(v, np.ndarray) else v.cpu().numpy())
            for k, v in st.items()}


def _batches(jobs):
    """jobs -> batches of 9 plans (7 working ones, pass-through plans in slots 2 and 6) and, for every tenth job, a batch of one."""
    out = []
    for b in range(0, len(jobs), 7):
        part = jobs[b:b + 7]
        slots = [None] * 9
        free = [s for s in range(9) if s not in (2, 6)]
        for s, j in zip(free, part):
            slots[s] = j
        out.append(slots)
    out += [[j] for j in jobs[::10]]
    return out


def _check_roll(st, x, shifts, n):
    """(a)"""
    for i, s in enumerate(shifts):
        assert np.array_equal(st["rolled"][i, :n], np.roll(x[i], s)), (i, s)
    assert np.all(st["rolled"][:, n:] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_stretch_stages(n):
    jobs = []
    for kind in KINDS:
        for rate in STRETCH_RATES:
            over = max(0, int(round(n / rate)) - n)
            for crop in sorted({0, over}):
                jobs.append((kind, rate, crop))
    clips = {k: _clip(k, n) for k in KINDS}
    for slots in _batches(jobs):
        x = np.stack([clips[j[0]] if j else clips["noise"] for j in slots])
        shifts = [(137 * (i + 1)) % n if i % 2 else 0 for i in range(len(slots))]
        plans = [dict(OFF, shift=shifts[i], rate=j[1], crop=j[2]) if j else dict(OFF, shift=shifts[i]) for i, j in enumerate(slots)]
        st = _stages(x, plans)
        _check_roll(st, x, shifts, n)
        assert np.array_equal(st["out"], st["stage"][:, :n]) and np.isfinite(st["out"]).all()
        for i, j in enumerate(slots):
            rec = st["records"][i]
            if j is None:
                assert rec["s_out"] == 0 and np.array_equal(st["out"][i], np.roll(x[i], shifts[i]))
                continue
            kind, rate, crop = j
            label = f"stretch n={n} B={len(slots)} {kind} rate={rate:.4f} crop={crop}"
            assert rec["s_rate"] == rate and rec["s_len"] == int(round(n / rate)) and rec["crop"] == crop
            rolled = st["rolled"][i, :n]
            fig, D, pv = check_magnitudes(st["S"][i], rolled, rate, label)
            FIGURES.append(dict(fig, n=n))
            FIGURES.append(dict(check_phase(st["S"][i], D, pv, fig["e_D"], label, require_share=kind in ("tonal", "noise")), n=n))
            FIGURES.append(dict(check_istft(st["S"][i], st["out"][i], int(rec["s_len"]), crop, label), n=n))


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_pitch_stages(n):
    rates = [ao.pitch_rate(s) for s in PITCH_STEPS] + [PITCH_RATE_EXACT, PITCH_RATE_NEAR]
    jobs = [(kind, r) for kind in KINDS for r in rates]
    clips = {k: _clip(k, n) for k in KINDS}
    for slots in _batches(jobs):
        x = np.stack([clips[j[0]] if j else clips["tonal"] for j in slots])
        shifts = [0 if i % 2 else -(211 * (i + 1)) % n for i in range(len(slots))]
        plans = [dict(OFF, shift=shifts[i], pitch_rate=j[1]) if j else dict(OFF, shift=shifts[i]) for i, j in enumerate(slots)]
        st = _stages(x, plans)
        _check_roll(st, x, shifts, n)
        assert np.array_equal(st["out"], st["stage"][:, :n]) and np.isfinite(st["out"]).all()
        for i, j in enumerate(slots):
            rec = st["records"][i]
            if j is None:
                assert rec["p_out"] == 0 and np.array_equal(st["out"][i], np.roll(x[i], shifts[i]))
                continue
            kind, rate = j
            label = f"pitch n={n} B={len(slots)} {kind} rate={rate:.4f}"
            ratio = 16000.0 / (16000.0 / rate)
            assert rec["p_rate"] == rate and rec["p_ratio"] == ratio and rec["p_len"] == int(round(n / rate))
            if rate in (PITCH_RATE_EXACT, PITCH_RATE_NEAR):
                assert ratio * 512 == (416.0 if rate == PITCH_RATE_EXACT else 479.99999999999994)
            assert np.isnan(st["Y_tail"][i]).all()                 # poisoned and never written: the finite outputs did not read it
            rolled, Y = st["rolled"][i, :n], st["Y"][i]
            fig, D, pv = check_magnitudes(st["S"][i], rolled, rate, label)
            FIGURES.append(dict(fig, n=n))
            FIGURES.append(dict(check_phase(st["S"][i], D, pv, fig["e_D"], label, require_share=kind in ("tonal", "noise")), n=n))
            FIGURES.append(dict(check_istft(st["S"][i], Y, int(rec["p_len"]), 0, label), n=n))
            FIGURES.append(dict(check_resample(Y, st["out"][i], ratio, int(rec["p_res"]), label), n=n))


@pytest.mark.gpu
@pytest.mark.parametrize("n", (5001, 16000))
def test_pitch_then_stretch_in_two_calls_equals_the_combined_call(n):
    """(g): the staged tests see one vocoder pass at a time; the trainer runs both in one call."""
    import torch
    from wakeword_jupyterlab_amd import ops
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(np.stack([_clip(k, n) for k in KINDS] + [_clip("tonal", n)] * 4)).to(dev)
    steps = [2.0, None, -3.0, 0.5, None, 3.0, -1.3, None, 1.0]
    rates = [0.7, 1.3, None, 0.91, None, 32 / 46, 1.0, 0.8, None]
    both = [dict(OFF, shift=97 * i, n_steps=steps[i], rate=rates[i], crop=max(0, int(round(n / rates[i])) - n) // 2 if rates[i] else 0,
                 sigma=0.1 * (i % 2), seed=i) for i in range(9)]
    first = [dict(p, rate=None, crop=0, sigma=0.0) for p in both]
    second = [dict(p, shift=0, n_steps=None) for p in both]
    got = ops.augment(ops.augment(x, first), second)
    assert torch.equal(got, ops.augment(x, both))
    with pytest.raises(ValueError):
        ops.augment_stages(x, both)
