"""logmel_cases.carry_batch, the batch of tests/test_gpu_logmel_carry.py, without a GPU: its coverage condition at three CU counts, its
repeatability, and what the oracle makes of the rows the GPU test looks at."""
import numpy as np
import pytest

import logmel_cases as lc

N = 4000          # the shortest clip: the row pattern does not depend on the length


@pytest.mark.parametrize("n_cu", [64, 256, 304])
def test_every_kind_follows_every_kind_at_every_grid(n_cu):
    """For each grid g in {1, 2, 3} x CUs and each ordered pair of kinds there is a row c of the first kind with row c + g of the second.
    carry_kinds asserts this itself; here it is checked from the returned kinds alone, with the counts."""
    B = lc.carry_rows(n_cu)
    assert B == 6 * n_cu + 41
    kinds = lc.carry_kinds(B, n_cu)
    assert len(kinds) == B and set(kinds) == set(lc.CARRY_KINDS)
    for m in (1, 2, 3):
        g = m * n_cu
        seen = {}
        for c in range(B - g):
            seen[kinds[c], kinds[c + g]] = seen.get((kinds[c], kinds[c + g]), 0) + 1
        assert len(seen) == 25 and min(seen.values()) >= 1, (n_cu, g, seen)
        assert B > 2 * g                                         # a workgroup of this grid takes a third clip somewhere
    # the period-3 pattern of the non-finite tests' batches does NOT have the property at the widest grid: the reason for this helper
    period3 = [("noisy", "tone", "noisy")[i % 3] for i in range(B)]
    assert all(period3[c] == period3[c + 3 * n_cu] for c in range(B - 3 * n_cu))


def test_the_batch_is_repeatable_and_made_as_described():
    n_cu = 64
    x, control, kinds = lc.carry_batch(N, n_cu)
    x2, control2, kinds2 = lc.carry_batch(N, n_cu)
    assert kinds == kinds2 and np.array_equal(x, x2, equal_nan=True) and np.array_equal(control, control2)
    assert x.shape == control.shape == (lc.carry_rows(n_cu), N) and x.dtype == control.dtype == np.float32
    kinds = np.array(kinds)
    assert np.isfinite(control).all() and np.abs(control).max(axis=1).min() > 0
    assert not np.isfinite(x[kinds == "special"]).all(axis=1).any() and not x[kinds == "silent"].any()
    same = np.isin(kinds, lc.ORDINARY_KINDS)
    assert np.array_equal(x[same], control[same]) and np.isfinite(x[same]).all()
    loud = np.abs(x[kinds == "loud"]).max(axis=1)
    assert loud.min() > 2.0 ** 12 and loud.max() < 2.0 ** 17      # a noisy clip (peak about 0.3 .. 1) times 2^15
    # all 17 non-finite cases occur
    cases = list(lc.nonfinite_cases(N).values())
    rows = x[kinds == "special"]
    assert all(any(np.array_equal(r, c, equal_nan=True) for r in rows[:len(cases)]) for c in cases)


@pytest.mark.parametrize("normalize", [True, False])
def test_oracle_on_the_sampled_rows(normalize):
    """The rows the GPU test holds to the oracle are finite images of levels in [-80, 0] dB; special rows are NaN in every element, and a
    silent row is NaN (0 / 0) with the normalisation and the flat 0 dB image without."""
    n_cu = 64
    x, _, kinds = lc.carry_batch(N, n_cu)
    plain, tone = lc.carry_sample_rows(kinds, n_cu)
    assert all(kinds[i] in ("noisy", "loud") for i in plain) and all(kinds[i] == "tone" for i in tone)
    assert {kinds[i] for i in plain} == {"noisy", "loud"}
    for mi, m in enumerate(lc.CARRY_GRIDS_PER_CU):
        for bi, before in enumerate(("special", "silent", "tone")):
            k = 3 * mi + bi
            assert kinds[plain[k] - m * n_cu] == before and kinds[tone[k] - m * n_cu] == before
    ref = lc.oracle_mel(x[plain + tone], N, normalize)
    assert ref.shape == (18, 1, 80, 1 + N // 512) and np.isfinite(ref).all()
    assert ref.min() >= -80.0 and ref.max() < 1e-3
    special = [i for i, k in enumerate(kinds) if k == "special"][:17]
    assert np.isnan(lc.oracle_mel(x[special], N, normalize)).all()
    silent = lc.oracle_mel(x[[kinds.index("silent")]], N, normalize)
    # (without: every value is the amin clamp under a reference level at the amin clamp, 0 dB up to the rounding of 10 log10(1e-10))
    assert np.isnan(silent).all() if normalize else np.abs(silent).max() <= 1e-4
