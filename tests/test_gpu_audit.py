"""The bank audit on the MI355X against tests/audit_ref.py: peak, clipped, non-finite count, hash and active
extent exactly; sum and sumsq within the float64 summation bound len * 2^-52 * sum |terms| of math.fsum (derived, not measured).  Before
an extent is compared the reference alone must show that no frame of the input lies within 1e-9 relative of the activity threshold.
Then duplicates, crop="active" on gathered windows, and the loader with and without it."""
import random

import numpy as np
import pytest
import torch

import audit_ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd.config import AudioConfig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N = 16000
TOP_DB, CLIP = 60.0, 0.999
CLIP32 = np.float32(CLIP)
EDGE_LENGTHS = [0, 1, 3, 511, 512, 513, 1023, 2047, 2048, 2049, 0, 16000, 16001, 7, 0]


def _proc(n=N):
    return pkg.AudioProcessor(type(f"AudioConfig{n}", (AudioConfig,), {"DURATION": n / 16000.0}), device=DEV)


def _noise(rng, n, db):
    return (rng.standard_normal(n) * 10.0 ** (db / 20.0) * 0.25).astype(np.float32)


def _split(x, lengths):
    at = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return [x[at[i]:at[i + 1]] for i in range(len(lengths))]


def _check(bank, xs, audit=None):
    """Every field of bank.audit() against the reference of the entries' samples `xs`."""
    ratio = audit_ref.ratio_of(TOP_DB)
    refs = [audit_ref.entry(x, ratio, CLIP) for x in xs]
    near = [(i, r["margin"]) for i, r in enumerate(refs) if r["margin"] <= 1e-9]
    assert not near, f"frames within 1e-9 of the activity threshold (pick another seed): {near}"
    au = bank.audit(TOP_DB, CLIP) if audit is None else audit
    assert len(au) == len(xs) == bank.n_entries and au.length.tolist() == [x.size for x in xs]
    assert np.array_equal(au.peak.view(np.uint32), bank.peaks.view(np.uint32))
    assert np.array_equal(au.peak.view(np.uint32), np.array([r["peak"] for r in refs], np.float32).view(np.uint32))
    assert au.clipped.tolist() == [r["clipped"] for r in refs]
    assert au.nonfinite.tolist() == [r["nonfinite"] for r in refs]
    assert au.hash.tolist() == [r["hash"] for r in refs]
    assert au.active_start.tolist() == [r["active_start"] for r in refs]
    assert au.active_end.tolist() == [r["active_end"] for r in refs]
    for i, (x, r) in enumerate(zip(xs, refs)):
        eps = x.size * 2.0 ** -52
        assert abs(au.sum[i] - r["sum"]) <= eps * r["abs_sum"], (i, au.sum[i], r["sum"])
        assert abs(au.sumsq[i] - r["sumsq"]) <= eps * r["abs_sumsq"], (i, au.sumsq[i], r["sumsq"])
        assert abs(au.max_frame_energy[i] - r["max_frame_energy"]) <= 2048 * 2.0 ** -52 * r["max_frame_energy"]
    return au, refs


def _edge_samples():
    rng = np.random.default_rng(21)
    levels = [-70, -60, -50, -40, -30, -20, -10, 0]
    return np.concatenate([_noise(rng, n, levels[i % 8]) for i, n in enumerate(EDGE_LENGTHS)] + [np.zeros(0, np.float32)])


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_edge_lengths_at_every_address_phase(shift):
    x = _edge_samples()
    buf = torch.full((x.size + 3 + 5,), 1e6, device=DEV)                 # what lies around the segment must not be looked at
    buf[shift:shift + x.size] = torch.from_numpy(x).to(DEV)
    b = pkg.ClipBank(_proc())
    b.add_buffer(buf[shift:shift + x.size], EDGE_LENGTHS)
    au, _ = _check(b, _split(x, EDGE_LENGTHS))
    assert au.hash[0] == au.hash[10] == au.hash[14] == 0 and au.peak[0] == 0 and (au.active_end[[0, 10, 14]] == 0).all()
    if shift:                                                            # the same bits wherever the segment lies
        b0 = pkg.ClipBank(_proc())
        b0.add_buffer(torch.from_numpy(x).to(DEV), EDGE_LENGTHS)
        assert b0.audit(TOP_DB, CLIP).stats.tobytes() == au.stats.tobytes()


def test_one_long_entry_folded_from_many_workgroups():
    rng = np.random.default_rng(22)
    x = _noise(rng, 300_000, -20)
    x[:100_000] *= np.float32(1e-4)                                      # 80 dB down: below the threshold
    x[250_000:] = 0.0
    b = pkg.ClipBank(_proc())
    b.add_buffer(torch.from_numpy(x).to(DEV), [x.size])
    au, _ = _check(b, [x])
    # sample 100,000 lies in hop block 195 and sample 249,999 in block 488; frame t sees the blocks t - 2 .. t + 1
    assert (au.active_start[0], au.active_end[0]) == (194 * 512, 491 * 512)


def test_more_entries_than_the_grid():
    rng = np.random.default_rng(23)
    lengths = rng.integers(1, 41, size=5000)
    x = _noise(rng, int(lengths.sum()), -10)
    b = pkg.ClipBank(_proc())
    b.add_buffer(torch.from_numpy(x).to(DEV), lengths)
    au, _ = _check(b, _split(x, lengths))
    assert (au.active_start == 0).all() and (au.active_end == lengths).all()


def _content_entries():
    rng = np.random.default_rng(24)
    xs = [_noise(rng, 4000 + 37 * i, db) for i, db in enumerate([-70, -60, -50, -40, -30, -20, -10, 0])]
    burst = np.zeros(48000, np.float32)
    burst[20000:26400] = rng.uniform(-0.9, 0.9, 6400).astype(np.float32)
    burst[23000] = 1.0                                                   # 0 dB
    xs.append(burst)
    xs.append(np.zeros(5000, np.float32))
    edge = _noise(rng, 3000, -20)
    below = np.nextafter(CLIP32, np.float32(0))
    edge[[5, 600, 1029]] = [CLIP32, -CLIP32, 1.0]                        # at the level exactly, and above: clipped
    edge[[6, 601, 2999]] = [below, -below, below]                        # one float32 step below: not
    xs.append(edge)
    bad = _noise(rng, 7001, -20)
    bad[[3, 4000]] = [np.nan, -np.inf]
    xs.append(bad)
    neg = _noise(rng, 2050, -30)
    neg[100:700] = -0.0
    xs.append(neg)
    xs.append(np.full(1000, -0.0, np.float32))
    return xs


def test_content_in_a_bank_of_two_segments():
    xs = _content_entries()
    b = pkg.ClipBank(_proc())
    b.add_buffer(torch.from_numpy(np.concatenate(xs[:9])).to(DEV), [x.size for x in xs[:9]], label=1)
    b.add_buffer(torch.from_numpy(np.concatenate(xs[9:])).to(DEV), [x.size for x in xs[9:]], label=0)
    assert len(b.segments) == 2
    au, refs = _check(b, xs)
    assert (au.active_start[8], au.active_end[8]) == (38 * 512, 54 * 512)            # the burst, widened to its frames
    assert (au.active_start[9], au.active_end[9]) == (0, 0) and au.rms_db[9] == -np.inf and au.hash[9] != 0
    assert au.clipped[10] == 3 and au.clipped[8] == 1
    assert au.nonfinite[11] == 2 and au.peak[11] == np.inf and (au.active_start[11], au.active_end[11]) == (0, 7001)
    assert np.isfinite(au.sum[11]) and np.isfinite(au.sumsq[11])
    assert au.hash[13] != audit_ref.content_hash(np.zeros(1000, np.float32)) and au.peak[13] == 0
    want_db = np.array([-70, -60, -50, -40, -30, -20, -10, 0]) + 20 * np.log10(0.25)
    assert np.abs(au.rms_db[:8] - want_db).max() < 0.5
    assert au.labels.tolist() == [1] * 9 + [0] * 5
    f = au.flags()
    assert np.flatnonzero(f.nonfinite).tolist() == [11] and np.flatnonzero(f.silent).tolist() == [0, 1, 2, 9, 13]
    assert np.flatnonzero(f.clipped).tolist() == [] and np.flatnonzero(au.flags(clipped_fraction=5e-4).clipped).tolist() == [10]
    assert "bank audit: 14 entries" in au.report()
    # two audits of the same memory are the same bytes; the cached one is returned until a segment is added
    assert b.audit(TOP_DB, CLIP) is au
    twin = pkg.ClipBank(_proc())
    twin.add_buffer(b.segments[0], [x.size for x in xs[:9]])
    twin.add_buffer(b.segments[1], [x.size for x in xs[9:]])
    assert twin.audit(TOP_DB, CLIP).stats.tobytes() == au.stats.tobytes()
    # another top_db moves the extents only
    refs5 = [audit_ref.entry(x, audit_ref.ratio_of(5.0), CLIP) for x in xs]
    assert min(r["margin"] for r in refs5) > 1e-9
    au5 = b.audit(5.0, CLIP)
    assert au5 is not au and np.array_equal(au5.hash, au.hash) and np.array_equal(au5.sumsq, au.sumsq)
    assert au5.active_start.tolist() == [r["active_start"] for r in refs5] and au5.active_end.tolist() == [r["active_end"] for r in refs5]
    assert au5.active_end[8] - au5.active_start[8] < au.active_end[8] - au.active_start[8]


def test_duplicates_on_the_device():
    rng = np.random.default_rng(25)
    x = _noise(rng, 5001, -12)
    y = x.copy()
    y[2500] = np.nextafter(y[2500], np.float32(1))                       # a near copy: one sample, one ulp
    pad = np.zeros(2, np.float32)
    lengths = [5001, 5001, 2, 5001, 5001]                                # x at address phases 0, 1 and 0; y at phase 1
    assert audit_ref.content_hash(x) != audit_ref.content_hash(y)
    b = pkg.ClipBank(_proc())
    b.add_buffer(torch.from_numpy(np.concatenate([x, x, pad, x, y])).to(DEV), lengths)
    au, _ = _check(b, [x, x, pad, x, y])
    assert au.hash[0] == au.hash[1] == au.hash[3] != au.hash[4]
    assert au.duplicates(verify=True) == [[0, 1, 3]] and au.duplicates(verify=False) == [[0, 1, 3]]
    val = pkg.ClipBank(_proc())
    val.add_buffer(torch.from_numpy(np.concatenate([y, pad, pad[:1], x])).to(DEV), [5001, 2, 1, 5001])
    for verify in (True, False):
        assert au.duplicates(verify=verify, other=val.audit()) == [([0, 1, 3], [3]), ([2], [1]), ([4], [0])]


def _burst_bank():
    rng = np.random.default_rng(26)
    x = np.zeros(3 * N, np.float32)
    x[20000:26400] = rng.choice(np.array([1.0, -1.0, 0.5, -0.5, 0.25, -0.25], np.float32), size=6400)   # squares that add exactly
    b = pkg.ClipBank(_proc())
    b.add_buffer(torch.from_numpy(x).to(DEV), [x.size], label=1)
    return b, float((x.astype(np.float64) ** 2).sum())


def test_active_crop_keeps_the_burst_in_every_window():
    b, want = _burst_bank()
    entries = np.zeros(200, np.int64)
    random.seed(31)
    starts = b.draw_starts(entries, crop="active")
    au = b.audit()
    assert (au.active_start[0], au.active_end[0]) == (38 * 512, 54 * 512)
    assert starts.min() >= 54 * 512 - N and starts.max() <= 38 * 512 and np.unique(starts).size > 100
    got = (b.gather(entries, starts, normalize=None).double() ** 2).sum(1).cpu().numpy()
    assert (got == want).all()
    random.seed(31)
    plain = b.draw_starts(entries)
    got = (b.gather(entries, plain, normalize=None).double() ** 2).sum(1).cpu().numpy()
    assert (got != want).any()                                           # the uniform rule does cut the burst: the test can tell


def _loader_bank():
    rng = np.random.default_rng(27)
    xs = [_noise(rng, n, -12) for n in (N, 2 * N + 11, N - 100, 3 * N, N + 1, 2 * N)]
    for x in xs[1::2]:
        x[: x.size // 3] = 0.0                                           # the longer ones start silent
    b = pkg.ClipBank(_proc())
    b.add_buffer(torch.from_numpy(np.concatenate(xs)).to(DEV), [x.size for x in xs], label=[1, 0, 1, 0, 1, 0])
    return b


def _epoch(loader, seed):
    random.seed(seed)
    torch.manual_seed(seed)
    return [(d.clone(), t.clone()) for d, t in loader]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(da.view(torch.int32), db.view(torch.int32)) and torch.equal(ta, tb)
                                    for (da, ta), (db, tb) in zip(a, b))


def test_loader_without_a_crop_is_unchanged_and_with_one_repeats():
    b = _loader_bank()
    base = _epoch(b.loader(4, shuffle=True, augment=True), seed=5)
    assert len(base) == 2 and _same(_epoch(b.loader(4, shuffle=True, augment=True, crop=None), seed=5), base)
    act = _epoch(b.loader(4, shuffle=True, augment=True, crop="active"), seed=5)
    assert _same(_epoch(b.loader(4, shuffle=True, augment=True, crop="active"), seed=5), act)
    assert [t.tolist() for _, t in act] == [t.tolist() for _, t in base] and not _same(act, base)     # same items, other windows
    with pytest.raises(ValueError):
        b.loader(4, crop="centre")
