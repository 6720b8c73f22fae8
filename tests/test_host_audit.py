"""The bank audit without a GPU: the start rule of crop="active" as a pure function, branch by branch and
over seeded draws; one draw per long entry; flags, report and duplicates on hand-made arrays; the argument checks of
ww_bank_audit_f32 / ww_bank_audit_workspace_bytes, which come before any device call; the record struct against the header; the
reference hash (tests/audit_ref.py) against values worked out by hand."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest
import torch

import audit_ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import audit as auditmod
from wakeword_jupyterlab_amd import bank as bankmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 16000


# ---- the start rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length, a, b, want", [
    (N - 1, 0, N - 1, (0, 0)),                          # len <= N: no draw, start 0
    (N, 512, 4096, (0, 0)),
    (0, 0, 0, (0, 0)),
    (3 * N, 0, 0, (0, 2 * N)),                          # no activity: the uniform window
    (3 * N, 0, 3 * N, (0, 2 * N)),                      # non-finite samples carry (0, len): uniform again
    (3 * N, 20000, 26400, (10400, 20000)),              # the region fits: b - N .. a
    (3 * N, 0, 6400, (0, 0)),                           # a = 0: the window must start at 0
    (3 * N, 512, 6400, (0, 512)),                       # b - N < 0 is clamped
    (3 * N, 3 * N - 6400, 3 * N, (2 * N, 2 * N)),       # b = len: the last window
    (3 * N, 3 * N - 6400, 3 * N - 512, (2 * N - 512, 2 * N)),   # a > len - N is clamped
    (3 * N, 10000, 10000 + N, (10000, 10000)),          # b - a = N exactly: one start, the region fills the window
    (3 * N, 10000, 10001 + N, (10000, 10001)),          # b - a > N: the window lies inside the region
    (3 * N, 0, 2 * N + 5, (0, N + 5)),
    (N + 1, 0, N + 1, (0, 1)),
])
def test_start_rule_branch_by_branch(length, a, b, want):
    lo, hi = auditmod.active_start_range([length], [a], [b], N)
    assert (int(lo[0]), int(hi[0])) == want


def test_start_rule_refuses_extents_outside_their_entries():
    for bad in (dict(lengths=[10], a=[0], b=[11]), dict(lengths=[10], a=[-1], b=[5]), dict(lengths=[-1], a=[0], b=[0]),
                dict(lengths=[10, 10], a=[0], b=[0])):
        with pytest.raises(ValueError):
            auditmod.active_start_range(n=4, **bad)
    with pytest.raises(ValueError):
        auditmod.active_start_range([10], [0], [5], 0)


def test_every_drawn_window_keeps_its_containment_property():
    rng = np.random.default_rng(4)
    lengths = rng.integers(N + 1, 5 * N, size=1000)
    a = (rng.integers(0, lengths) // 512) * 512
    width = rng.choice([512, 4096, N - 512, N, N + 512, 3 * N], size=1000)
    b = np.minimum(lengths, a + width)
    lo, hi = auditmod.active_start_range(lengths, a, b, N)
    assert (lo <= hi).all() and (lo >= 0).all() and (hi <= lengths - N).all()
    random.seed(4)
    seen_fit = seen_inside = 0
    for i in range(1000):
        s = random.randint(int(lo[i]), int(hi[i]))
        if b[i] - a[i] <= N:
            assert s <= a[i] and b[i] <= s + N                       # the window holds the whole active region
            seen_fit += 1
        else:
            assert a[i] <= s and s + N <= b[i]                       # the window lies inside the active region
            seen_inside += 1
    assert seen_fit > 100 and seen_inside > 100


# ---- draw_starts and the loader, against a stand-in gather and a stand-in audit --------------------------------------------------------
class _Proc:
    config = pkg.AudioConfig
    device = None

    def _check_augment(self):
        pass

    def augment_batch(self, pcm):
        return pcm

    def mel_batch(self, pcm, normalize=True):
        return pcm[:, None, :80, None].repeat(1, 1, 1, 32).clone()


def _bank():
    b = pkg.ClipBank(_Proc())
    lens = np.array([N - 1, 3 * N, 0, N, 3 * N, 3 * N, 2 * N], np.int64)
    b._add_segment(torch.zeros(int(lens.sum())), lens, bankmod.CLIP, [1, 1, 0, 0, 1, 0, 1], ok=[True, True, False, True, True, True, True],
                   peaks=np.ones(lens.size, np.float32))
    b._add_segment(torch.zeros(10 * N), [10 * N], bankmod.STREAM, 0, peaks=np.ones(1, np.float32))
    #              entry:    0      1      2  3      4           5      6         7 (stream: its extent must be ignored)
    a = np.array([0,     20000, 0, 0, 5120,           0, 0,         512])
    e = np.array([N - 1, 26400, 0, N, 5120 + 2 * N,   0, 2 * N,     1024])
    b._audits[(60.0, float(np.float32(0.999)))] = pkg.BankAudit.from_stats(b.lengths, N, active_start=a, active_end=e, labels=b.labels,
                                                                            ok=b.ok, kinds=b.kinds)
    b._gather = lambda entries, starts, norms, out=None, rows=None: torch.zeros(len(entries), N)
    return b


def test_active_crop_draws_once_per_long_entry_in_the_rules_range(monkeypatch):
    b = _bank()
    entries = np.array([7, 0, 1, 2, 3, 4, 5, 6, 1])
    random.seed(9)
    got = b.draw_starts(entries, crop="active")
    state = random.getstate()
    random.seed(9)
    want = [random.randint(0, 9 * N), 0, random.randint(10400, 20000), 0, 0, random.randint(5120, 5120 + N), random.randint(0, 2 * N),
            random.randint(0, N), random.randint(10400, 20000)]
    assert got.tolist() == want
    assert random.getstate() == state                                # exactly one draw per entry longer than N, as without a crop
    random.seed(9)
    plain = b.draw_starts(entries)
    assert plain.tolist() != got.tolist()
    random.seed(9)
    assert b.draw_starts(entries, crop=None).tolist() == plain.tolist()
    calls = []
    monkeypatch.setattr(random, "randint", lambda lo, hi: calls.append((lo, hi)) or lo)
    b.draw_starts(entries, crop="active")
    n_active, calls[:] = len(calls), []
    b.draw_starts(entries)
    assert n_active == len(calls) == 6 == int((b.lengths[entries] > N).sum())          # (a rejection inside randint may still move the state)


def test_crop_values_are_checked_at_construction():
    b = _bank()
    for bad in ("Active", "center", True, 0):
        with pytest.raises(ValueError):
            b.loader(4, crop=bad)
        with pytest.raises(ValueError):
            bankmod.BankLoader(b, 4, crop=bad)
        with pytest.raises(ValueError):
            b.draw_starts(np.array([1]), crop=bad)
    assert b.loader(4).crop is None and b.loader(4, crop="active").crop == "active"
    random.seed(2)
    torch.manual_seed(2)
    assert sum(d.shape[0] for d, _ in b.loader(4, shuffle=True, crop="active")) == b.n_items


def test_an_audit_is_dropped_when_a_segment_is_added():
    b = _bank()
    assert b._audits
    b._add_segment(torch.zeros(8), [8], bankmod.CLIP, 0, peaks=np.ones(1, np.float32))
    assert b._audits == {}


# ---- flags, report, duplicates on hand-made arrays ------------------------------------------------------------------------------------
def _audit():
    #                  0 fine   1 silent  2 clipped  3 dc      4 short   5 overlong  6 nonfinite  7 empty  8 unreadable  9 all zero
    length = np.array([16000,   16000,    16000,     16000,    16000,    48000,      16000,       0,       0,            16000])
    sumsq = np.array([160.0,    1.6e-4,   8000.0,    160.0,    160.0,    480.0,      1.0,         0.0,     0.0,          0.0])
    total = np.array([0.0,      0.0,      0.0,       400.0,    0.0,      0.0,        0.0,         0.0,     0.0,          0.0])
    return pkg.BankAudit.from_stats(
        length, N, sum=total, sumsq=sumsq, peak=np.array([0.5, 1e-3, 1.0, 0.5, 0.5, 0.5, np.inf, 0, 0, 0], np.float32),
        clipped=[0, 0, 17, 0, 16, 0, 0, 0, 0, 0], nonfinite=[0, 0, 0, 0, 0, 0, 2, 0, 0, 0],
        active_start=[0, 0, 0, 0, 4096, 1024, 0, 0, 0, 0], active_end=[16000, 16000, 16000, 16000, 6144, 40960, 16000, 0, 0, 0],
        hash=[11, 12, 13, 11, 15, 16, 17, 0, 0, 11], labels=[1, 1, 1, 0, 0, 1, 0, 0, 1, 0],
        ok=[True, True, True, True, True, True, True, True, False, True])


def test_derived_levels():
    au = _audit()
    assert au.rms_db[0] == pytest.approx(-20.0) and au.rms_db[1] == pytest.approx(-80.0) and au.rms_db[9] == -np.inf and au.rms_db[7] == -np.inf
    assert au.dc[3] == pytest.approx(0.025) and au.crest_db[0] == pytest.approx(20 * np.log10(0.5 / 0.1)) and np.isnan(au.crest_db[9])
    assert au.rms_db[6] == pytest.approx(10 * np.log10(1.0 / 15998))          # over the finite samples
    assert len(au) == 10 and au.peak.dtype == np.float32 and au.hash.dtype == np.uint64


def test_flags_follow_the_policy_and_its_arguments():
    f = _audit().flags()
    want = {"unreadable": [8], "empty": [7], "silent": [1, 9], "clipped": [2], "dc_offset": [3], "short": [4], "overlong": [5], "nonfinite": [6]}
    for k, idx in want.items():
        assert np.flatnonzero(getattr(f, k)).tolist() == idx, k
    assert np.flatnonzero(f.any).tolist() == list(range(1, 10)) and f.counts()["silent"] == 2
    au = _audit()
    assert np.flatnonzero(au.flags(silent_db=-90.0).silent).tolist() == [9]             # all zeros have no active frame at any level
    assert np.flatnonzero(au.flags(clipped_fraction=1e-4).clipped).tolist() == [2, 4]    # 16 of 16000 = 1e-3 is not MORE than 1e-3
    assert np.flatnonzero(au.flags(dc=0.03).dc_offset).tolist() == []
    assert np.flatnonzero(au.flags(min_active=0.1).short).tolist() == []                 # 2048 samples = 0.128 s
    assert np.flatnonzero(au.flags(min_active=1.5).short).tolist() == [0, 2, 3, 4]


def test_report_counts_flags_per_label_and_lists_the_worst():
    text = _audit().report(worst=1)
    assert "bank audit: 10 entries" in text and "entries per label: 0: 5, 1: 5" in text and "flagged: 9 of 10" in text
    lines = text.splitlines()
    row = {ln.split()[0]: ln for ln in lines if ln.startswith("  ") and not ln.startswith("      ")}
    assert set(row) == set(auditmod.FLAG_NAMES)
    assert row["silent"].split()[1] == "2" and "0: 1, 1: 1" in row["silent"]
    assert row["nonfinite"].split()[1] == "1" and "0: 1, 1: 0" in row["nonfinite"]
    at = lines.index(row["silent"])
    assert lines[at + 1].startswith("      entry 9:") and not lines[at + 2].startswith("      ")     # the all-zero entry is the quietest
    assert "entry 5: label 1, 3.000 s" in text and "active 0.064-2.560 s" in text
    assert len(_audit().report(worst=0).splitlines()) == 3 + len(auditmod.FLAG_NAMES)


def test_duplicates_group_by_length_and_hash():
    au = _audit()
    assert au.duplicates(verify=False) == [[0, 3, 9]]                 # hash 11 three times at one length; the empty entries never group
    with pytest.raises(ValueError):
        au.duplicates()                                              # verify needs the samples
    other = pkg.BankAudit.from_stats([16000, 16000, 48000, 0], N, hash=[13, 99, 16, 0])
    assert au.duplicates(verify=False, other=other) == [([2], [0]), ([5], [2])]
    assert other.duplicates(verify=False, other=au) == [([0], [2]), ([2], [5])]


def test_duplicates_verify_compares_the_samples():
    b = pkg.ClipBank(_Proc())
    x = np.arange(40, dtype=np.float32)
    y = x.copy()
    y[7] = np.nextafter(y[7], np.float32(np.inf))
    data = np.concatenate([x, y, x, [-0.0] * 40, [0.0] * 40]).astype(np.float32)
    b._add_segment(torch.from_numpy(data), [40] * 5, bankmod.CLIP, 0, peaks=np.ones(5, np.float32))
    au = pkg.BankAudit.from_stats(b.lengths, N, hash=[5, 5, 5, 6, 6], bank=b)           # as if y collided with x, and -0.0 with +0.0
    assert au.duplicates(verify=False) == [[0, 1, 2], [3, 4]]
    assert au.duplicates(verify=True) == [[0, 2]]
    assert au.duplicates(verify=True, other=au) == [([0, 2], [0, 2]), ([1], [1]), ([3], [3]), ([4], [4])]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def _call(audio, total, off_dev, off_host, n, clip=0.999, ratio=1e-6, stats=None, ws=None):
    host = None if off_host is None else np.asarray(off_host, np.int64)
    return nat.lib.ww_bank_audit_f32(audio, total, off_dev, None if host is None else host.ctypes.data, n, clip, ratio, stats, ws, None)


def test_audit_argument_checks_come_before_the_device():
    buf = np.zeros(1024, np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data % 256)
    err = nat.lib.ww_last_error
    ok_off = [0, 10, 10, 40]
    assert _call(p, -1, p, ok_off, 3, stats=p, ws=p) == nat.WW_EINVAL and b"total_samples" in err()
    assert _call(p, 40, p, ok_off, -1, stats=p, ws=p) == nat.WW_EINVAL and b"n_entries" in err()
    for clip in (0.0, -1.0, float("nan")):
        assert _call(p, 40, p, ok_off, 3, clip=clip, stats=p, ws=p) == nat.WW_EINVAL and b"clip_level" in err()
    for ratio in (0.0, -1e-3, 1.0000001, float("nan"), float("inf")):
        assert _call(p, 40, p, ok_off, 3, ratio=ratio, stats=p, ws=p) == nat.WW_EINVAL and b"ratio" in err()
    assert _call(p, 40, p, None, 3, stats=p, ws=p) == nat.WW_EINVAL and b"offsets_host" in err()
    assert _call(p, 40, p, [0, 10, 9, 40], 3, stats=p, ws=p) == nat.WW_EINVAL and b"non-decreasing" in err()
    assert _call(p, 40, p, [-1, 10, 10, 40], 3, stats=p, ws=p) == nat.WW_EINVAL and b"offsets[0]" in err()
    assert _call(p, 39, p, ok_off, 3, stats=p, ws=p) == nat.WW_EINVAL and b"passes total_samples" in err()
    for kw in (dict(audio=None), dict(off_dev=None), dict(stats=None), dict(ws=None)):
        args = dict(audio=p, off_dev=p, stats=p, ws=p)
        args.update(kw)
        assert _call(args["audio"], 40, args["off_dev"], ok_off, 3, stats=args["stats"], ws=args["ws"]) == nat.WW_EINVAL and b"null" in err()
    assert _call(p + 2, 40, p, ok_off, 3, stats=p, ws=p) == nat.WW_EINVAL and b"aligned" in err()
    assert _call(p, 40, p + 4, ok_off, 3, stats=p, ws=p) == nat.WW_EINVAL and b"aligned" in err()
    assert _call(p, 40, p, ok_off, 3, stats=p + 4, ws=p) == nat.WW_EINVAL and b"aligned" in err()
    assert _call(p, 40, p, ok_off, 3, stats=p, ws=p + 128) == nat.WW_EINVAL and b"aligned" in err()
    assert _call(None, 0, None, None, 0) == nat.WW_OK                                     # nothing to do
    assert _call(None, 0, None, None, 0, ratio=2.0) == nat.WW_EINVAL                      # the scalars are checked even then
    if not torch.cuda.is_available():                                                     # every check passed; no device here
        assert _call(p, 40, p, ok_off, 3, stats=p, ws=p) == nat.WW_ENODEVICE
        assert _call(p, 40, p, ok_off, 3, ratio=1.0, stats=p, ws=p) == nat.WW_ENODEVICE   # ratio = 1 is allowed


def test_workspace_bytes():
    ws = nat.lib.ww_bank_audit_workspace_bytes
    assert ws(-1, 1) == nat.WW_EINVAL and b"total_samples" in nat.lib.ww_last_error()
    assert ws(10, -1) == nat.WW_EINVAL and ws(10, (1 << 30) + 1) == nat.WW_EINVAL and b"n_entries" in nat.lib.ww_last_error()
    assert ws(0, 0) == 256 + 256                                     # the hop table's last value, and room for one record
    # a prefix table of n + 1 int64 and one 40-byte record per hop block, at most total / 512 + n of them, each part rounded to 256
    assert ws(16000 * 100, 100) == 1024 + -(-(3125 + 100 + 1) * 40 // 256) * 256
    assert ws(1 << 33, 3) % 256 == 0 and ws(1 << 33, 3) > (1 << 24) * 40


def test_stats_struct_is_the_headers():
    text = open(os.path.join(ROOT, "include", "wakeword_amd.h")).read()
    body = re.search(r"typedef struct ww_bank_entry_stats \{(.*?)\} ww_bank_entry_stats;", text, flags=re.S).group(1)
    fields = re.findall(r"(double|int64_t|uint64_t|int32_t|float)\s+(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    ctype = {"double": C.c_double, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "int32_t": C.c_int32, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(nat.BankEntryStats._fields_)
    assert [n for _, n in fields] == list(auditmod.STATS_DTYPE.names)
    assert [auditmod.STATS_DTYPE.fields[n][1] for _, n in fields] == [getattr(nat.BankEntryStats, n).offset for _, n in fields]
    assert C.sizeof(nat.BankEntryStats) == auditmod.STATS_DTYPE.itemsize == 72
    assert re.search(r"#define WW_AUDIT_HOP 512\b", text) and nat.AUDIT_HOP == audit_ref.HOP == 512
    assert re.search(r"#define WW_AUDIT_FRAME 2048\b", text) and nat.AUDIT_FRAME == 2048


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------
def test_reference_hash_against_hand_computed_values():
    # +0.0f at index 0: m = 0, k1 = 0 -> fmix32 = 0; k2 = 0x27D4EB2F -> fmix32 = 0x8C03471F
    assert audit_ref.content_hash(np.array([0.0], np.float32)) == 0x8C03471F00000000
    # 1.0f = 0x3F800000 at index 1: m = 0x9E3779B1, k1 = 0xA1B779B1 -> 0x41FE67E4; rotl(m, 15) = 0xBCD8CF1B, k2 = 0x242DBA4A -> 0x7BE278AC
    assert int(audit_ref.mix(np.uint32(0x3F800000), np.uint64(1))) == 0x7BE278AC41FE67E4
    assert audit_ref.content_hash(np.array([0.0, 1.0], np.float32)) == 0x07E5BFCB41FE67E4            # their wrapping sum
    assert audit_ref.content_hash(np.array([1.0], np.float32), first_index=1) == 0x7BE278AC41FE67E4   # partial sums combine
    # -0.0f at index 2^32 + 2: the high word of the index takes part
    assert int(audit_ref.mix(np.uint32(0x80000000), np.uint64((1 << 32) + 2))) == 0x399ADE52A88C5762
    assert audit_ref.content_hash(np.zeros(0, np.float32)) == 0
    x = np.random.default_rng(0).standard_normal(1000).astype(np.float32)
    parts = sum(audit_ref.content_hash(x[i:i + 100], first_index=i) for i in range(0, 1000, 100)) % (1 << 64)
    assert parts == audit_ref.content_hash(x) != audit_ref.content_hash(x[::-1])


def test_reference_activity_rule_on_a_burst():
    x = np.zeros(48000, np.float32)
    x[20000:26400] = 0.5                                             # blocks 39 .. 51 hold it (26400 = 51.56 blocks)
    r = audit_ref.entry(x, audit_ref.ratio_of(60.0), 0.999)
    # frame t sees blocks t - 2 .. t + 1: the first with energy is t = 38, the last t = 53
    assert (r["active_start"], r["active_end"]) == (38 * 512, 54 * 512) and r["nonfinite"] == 0 and r["clipped"] == 0
    assert r["sumsq"] == 6400 * 0.25 and r["peak"] == np.float32(0.5)
    assert audit_ref.entry(np.zeros(100, np.float32), 1e-6, 0.999)["active_end"] == 0
    x[5] = np.nan
    assert (audit_ref.entry(x, 1e-6, 0.999)["active_start"], audit_ref.entry(x, 1e-6, 0.999)["active_end"]) == (0, 48000)
