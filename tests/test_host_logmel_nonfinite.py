"""Non-finite samples and signal level in the log-mel front-end, without a GPU: what the oracle gives for the shared cases of
tests/logmel_cases.py (the expectation tests/test_gpu_logmel_nonfinite.py holds the kernels to), and the teeth of its row checker: a
numpy stand-in of the float kernel's epilogue as it was (fmax folds that drop a NaN) must fail it, the NaN-sticky one must pass."""
import numpy as np
import pytest

import logmel_cases as lc


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("n", [16000, 4000])
def test_oracle_gives_an_all_nan_image_for_every_case(n, normalize):
    cases = lc.nonfinite_cases(n)
    ref = lc.oracle_mel(list(cases.values()), n, normalize)
    assert ref.shape == (len(cases), 1, 80, 1 + n // 512)
    for name, img in zip(cases, ref):
        assert np.isnan(img).all(), (name, int(np.isfinite(img).sum()))


def test_oracle_gives_an_all_nan_image_for_short_rows():
    cases = lc.nonfinite_cases(16000, valid=9000)
    ref = lc.oracle_mel(list(cases.values()), 16000, True)
    assert np.isnan(ref).all()


def _batch(n, names):
    """Special clips at rows 0, 2, ... and the last, noisy clips between them; and the control batch."""
    cases = lc.nonfinite_cases(n)
    rows, special = [], []
    for j, name in enumerate(names):
        special.append(len(rows))
        rows.append(cases[name])
        rows.append(lc.noisy(40 + j, n))
    special.append(len(rows))
    rows.append(cases[names[0]])
    control = [lc.noisy(900 + i, n) if i in special else r for i, r in enumerate(rows)]
    return rows, special, control


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("n", [16000, 4000])
def test_row_checker_rejects_the_dropping_fold_and_accepts_the_sticky_one(n, normalize):
    names = ["nan@0", "nan@512", "nan@last", "two_nans_apart", "+inf", "-inf", "nan_in_tone"]
    rows, special, control = _batch(n, names)
    ctl = lc.standin_logmel(control, n, normalize, sticky=False)
    assert np.isfinite(ctl).all()
    assert np.array_equal(ctl, lc.standin_logmel(control, n, normalize, sticky=True))      # finite clips keep their bits
    old = lc.standin_logmel(rows, n, normalize, sticky=False)
    with pytest.raises(AssertionError, match="are not NaN"):
        lc.check_rows(old, special, ctl)
    # what the dropped NaN leaves behind: only the frames that cover the sample are NaN, the others are ordinary dB values
    T = 1 + n // 512
    img = old[special[1]][0]                       # nan@512: frames 0 .. 2 hold sample 512 (|512 - 512 t| < 1024), frame 3 has w[0] = 0 there
    nan_cols = np.isnan(img).all(axis=0)
    assert nan_cols[:3].all() and not np.isnan(img[:, 4:]).any() and nan_cols.sum() in (3, 4)
    assert np.isfinite(img[:, 4:]).all() and img[:, 4:].max() == 0.0 and T - nan_cols.sum() >= 4
    new = lc.standin_logmel(rows, n, normalize, sticky=True)
    lc.check_rows(new, special, ctl)
    # and a leak into a neighbour is caught too
    leaked = new.copy()
    leaked[1, 0, 79, T - 1] = np.nextafter(leaked[1, 0, 79, T - 1], np.float32(1))
    with pytest.raises(AssertionError, match="ordinary row 1"):
        lc.check_rows(leaked, special, ctl)


@pytest.mark.parametrize("n", [16000, 4000])
def test_dropping_fold_turns_an_inf_sample_into_a_flat_0_db_image(n):
    """normalize=True: the peak is Inf, g2 = 0, the NaN powers are dropped from the maximum and the reference level clamps to amin:
    every frame the sample does not touch reads exactly 0 dB -- finite, plausible and entirely wrong."""
    x = lc.nonfinite_cases(n)["+inf"]
    img = lc.standin_logmel([x], n, True, sticky=False)[0, 0]
    at = int(np.flatnonzero(np.isinf(x))[0])
    untouched = np.abs(512 * np.arange(1 + n // 512) - at) > 1024
    assert untouched.sum() >= 3
    assert np.all(img[:, untouched] == 0.0)
    assert np.isnan(img[:, ~untouched]).all()
    assert np.isnan(lc.standin_logmel([x], n, True, sticky=True)).all()


@pytest.mark.parametrize("n", [16000, 4000, 32000])
def test_oracle_is_bit_equal_under_power_of_two_gains(n):
    x = np.stack([lc.noisy(3, n), lc.noisy(4, n), lc.tones(n)[1]])
    ref = lc.oracle_mel(x, n, True)
    assert np.isfinite(ref).all()
    for k in lc.POW2_GAINS + lc.POW2_GAINS_F64:
        assert np.array_equal(lc.oracle_mel(lc.scaled(x, k), n, True), ref), k
