"""The clip ledger without a GPU: the layout of the record, the host side of the ww_clip_ledger_* entry points,
every number of ledger.LedgerReport against the brute force of tests/ledger_ref.py, and the `entries=` argument of bank.loader."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ledger_ref as ref
import test_host_bank as hb
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import ledger as led
from wakeword_jupyterlab_amd.ledger import LedgerReport

HAS_GPU = torch.cuda.is_available()


def test_layout_is_the_headers():
    assert C.sizeof(nat.LedgerHeader) == led.HEADER_BYTES == 64 and C.sizeof(nat.LedgerEntry) == led.ENTRY_DTYPE.itemsize == 56
    assert [f[0] for f in nat.LedgerHeader._fields_] == list(led.HEADER_FIELDS) == list(ref.HEADER_FIELDS)
    for name, _ in nat.LedgerEntry._fields_:
        assert getattr(nat.LedgerEntry, name).offset == led.ENTRY_DTYPE.fields[name][1], name
    assert pkg.ClipLedger is led.ClipLedger and pkg.LedgerReport is LedgerReport
    f = nat.lib.ww_clip_ledger_bytes
    assert f(0) == 64 and f(1) == 120 and f(300) == 64 + 56 * 300 and f(1 << 28) == 64 + 56 * (1 << 28)
    for bad in (-1, (1 << 28) + 1, 1 << 40):
        assert f(bad) == nat.WW_EINVAL and b"n_entries" in nat.lib.ww_last_error()
    assert nat.lib.ww_abi_version() == 4


def test_argument_checks_return_einval_before_any_hip_call():
    buf = np.zeros(64, np.int64)
    base = buf.ctypes.data
    upd, init = nat.lib.ww_clip_ledger_update_f32, nat.lib.ww_clip_ledger_init

    def einval(rc, word):
        assert rc == nat.WW_EINVAL and word in nat.lib.ww_last_error(), (rc, nat.lib.ww_last_error())
    ok = dict(logits=base, labels=base, entries=base, n=4, epoch=0, ledger=base, n_entries=3)

    def call(**kw):
        a = dict(ok, **kw)
        return upd(a["logits"], a["labels"], a["entries"], a["n"], a["epoch"], a["ledger"], a["n_entries"], None)
    einval(call(logits=None), b"null logits_dev")
    einval(call(labels=None), b"null logits_dev / labels_dev")
    einval(call(entries=None), b"entries_dev pointer")
    einval(call(ledger=None), b"null ledger_dev")
    einval(call(logits=base + 4), b"logits_dev must be 8-byte")
    einval(call(labels=base + 4), b"labels_dev must be 8-byte")
    einval(call(entries=base + 4), b"entries_dev must be 8-byte")
    einval(call(ledger=base + 4), b"ledger_dev must be 8-byte")
    einval(call(n=-1), b"n -1")
    einval(call(n=(1 << 30) + 1), b"n ")
    einval(call(n_entries=-1), b"n_entries -1")
    einval(call(n_entries=(1 << 28) + 1), b"n_entries ")
    einval(call(epoch=-2), b"epoch -2")
    einval(call(epoch=64), b"epoch 64")
    einval(call(n=0, ledger=base + 4), b"ledger_dev must be 8-byte")          # the checks come before the n == 0 return
    einval(call(n=0, epoch=99), b"epoch 99")
    assert call(n=0) == nat.WW_OK and call(n=0, epoch=-1) == nat.WW_OK and call(n=0, epoch=63) == nat.WW_OK   # nothing to launch
    einval(init(None, 3, None), b"null ledger_dev")
    einval(init(base + 2, 3, None), b"ledger_dev must be 8-byte")
    einval(init(base, -1, None), b"n_entries -1")
    einval(init(base, (1 << 28) + 1, None), b"n_entries ")
    if not HAS_GPU:                                                            # valid arguments: only the device is missing
        assert call() == nat.WW_ENODEVICE and call(epoch=-1) == nat.WW_ENODEVICE and init(base, 3, None) == nat.WW_ENODEVICE
        assert init(base, 0, None) == nat.WW_ENODEVICE
    assert not buf.any()                                                       # and nothing was written


# ---- LedgerReport against the brute force -----------------------------------------------------------------------------------------
def _report(r: ref.RefLedger) -> LedgerReport:
    return LedgerReport.from_buffer(r.tobytes(), r.n_entries)


def _check_against_visits(rep, r, fast_std=()):
    for e in range(r.n_entries):
        v = r.visits[e]
        assert rep.seen[e] == len(v) and rep.seen_finite[e] == len([q for _, _, q in v if q is not None])
        for name in ("mean_margin", "min_margin", "max_margin", "accuracy"):
            got, want = float(getattr(rep, name)[e]), getattr(ref, name)(v)
            assert (math.isnan(got) and math.isnan(want)) or got == want, (name, e, got, want)
        want_std = ref.std_margin_fast(v) if e in fast_std else ref.std_margin(v)
        assert ref.close(float(rep.std_margin[e]), want_std), (e, float(rep.std_margin[e]), want_std)
        assert rep.learned_epoch[e] == ref.learned_epoch(v) and rep.forgetting[e] == ref.forgetting(v), e
        assert bool(rep.never_learned[e]) == ref.never_learned(v), e


def _rows(margins, labels):
    """Logits whose margin of class 1 is exactly `margins` (z0 = 0)."""
    m = np.asarray(margins, np.float32)
    return np.stack([np.zeros_like(m), m], axis=1), np.asarray(labels, np.int64)


def _hand_built():
    """Entry 0: sum_q2 near 2^60 (70000 visits at the clamp, both signs).  1: seen only in epochs 0 and 63.  2: only non-finite visits.
    3: right, wrong, unseen, right, wrong over epochs 0..4 (plus a second forgetting later).  4: never seen.  5: wrong in every epoch it was
    seen in.  6: seen under epoch -1 only.  7: two visits in one epoch, one right and one wrong, then right."""
    r = ref.RefLedger(8)
    z, y = _rows(np.concatenate([np.full(40000, 100.0), np.full(30000, -80.0)]), np.ones(70000))
    r.update(z, y, np.zeros(70000, np.int64), 5)
    r.update(*_rows([3.25], [1]), [1], 0)
    r.update(*_rows([-0.5], [0]), [1], 63)
    for ep, m in ((1, np.nan), (2, np.inf), (2, -np.inf)):
        r.update(*_rows([m], [1]), [2], ep)
    for ep, m in ((0, 1.5), (1, -0.25), (3, 2.0), (4, -1.0), (9, 0.125), (10, 0.5), (40, -3.0)):
        r.update(*_rows([m], [1]), [3], ep)
    for ep in (2, 7, 33):
        r.update(*_rows([0.75], [0]), [5], ep)
    r.update(*_rows([1.0, -1.0, 0.0], [1, 1, 0]), [6, 6, 6], -1)
    r.update(*_rows([2.0, -2.0], [1, 1]), [7, 7], 12)
    r.update(*_rows([2.5], [1]), [7], 13)
    return r


def test_report_arithmetic_matches_the_brute_force_on_hand_built_ledgers():
    r = _hand_built()
    rep = _report(r)
    assert rep.tobytes() == r.tobytes() and rep == _report(r)
    _check_against_visits(rep, r, fast_std={0})
    # the cases by hand
    assert int(rep.sum_q2[0]) == 70000 * (1 << 44) and 2 ** 60 < int(rep.sum_q2[0]) < 2 ** 61           # n * sum_q2 overflows int64
    assert rep.min_margin[0] == -64.0 and rep.max_margin[0] == 64.0 and rep.mean_margin[0] == 64.0 * 10000 / 70000
    assert ref.close(float(rep.std_margin[0]), 64.0 * math.sqrt(1.0 - (1.0 / 7.0) ** 2))
    assert rep.seen_epochs[1] == (1 | 1 << 63) and rep.learned_epoch[1] == 0 and rep.forgetting[1] == 0
    assert rep.mean_margin[1] == (3.25 + 0.5) / 2                                                       # label 0: the margin is -d
    assert rep.seen[2] == rep.nonfinite[2] == 3 and rep.seen_finite[2] == 0 and math.isnan(rep.mean_margin[2]) and math.isnan(rep.std_margin[2])
    assert math.isnan(rep.min_margin[2]) and rep.min_q[2] == ref.INT32_MAX and rep.max_q[2] == ref.INT32_MIN
    assert rep.accuracy[2] == 1.0 / 3.0                                                                 # +inf is right, NaN and -inf are wrong
    assert rep.learned_epoch[3] == 0 and rep.forgetting[3] == 3 and not rep.never_learned[3]
    assert rep.seen[4] == 0 and math.isnan(rep.accuracy[4]) and rep.learned_epoch[4] == -1 and not rep.never_learned[4]
    assert rep.never_learned[5] and rep.learned_epoch[5] == -1 and rep.correct[5] == 0
    assert rep.seen[6] == 3 and rep.seen_epochs[6] == 0 and not rep.never_learned[6] and rep.correct[6] == 2   # the tie predicts 0: right
    assert rep.learned_epoch[7] == 13 and rep.forgetting[7] == 0 and rep.wrong_epochs[7] == 1 << 12
    assert rep.header["rows"] == 70000 + 2 + 3 + 7 + 3 + 3 + 3 and rep.header["nonfinite"] == 3 and rep.header["updates"] == 19
    # flags and what follows from them
    f = rep.flags()
    assert sorted(f) == sorted(led.FLAG_NAMES)
    assert f["unseen"].tolist() == [False] * 4 + [True] + [False] * 3
    assert f["suspect"].tolist() == [False, False, False, True, False, True, False, False]              # 3: mean -0.125 / 7, 5: -0.75
    assert f["never_learned"].tolist() == [True, False, True, False, False, True, False, False]    # 0 and 2: each of their epochs holds a wrong visit
    assert f["forgotten"].tolist() == [False, False, False, True, False, False, False, False]
    assert f["nonfinite"].tolist() == [False, False, True] + [False] * 5
    assert rep.suspects().tolist() == [5, 3] and rep.suspects(1).tolist() == [5] and rep.suspects(min_seen=4).tolist() == [3]
    assert rep.flags(min_seen=8)["suspect"].sum() == 0
    assert rep.misclassified().tolist() == [0, 2, 3, 5, 6, 7]
    assert rep.keep().tolist() == (~f["suspect"]).tolist()
    assert rep.keep(drop=("suspect", "nonfinite", "unseen")).tolist() == [True, True, False, False, False, False, True, True]
    assert rep.keep(drop="never_learned", min_seen=2).tolist() == (~f["never_learned"]).tolist()
    with pytest.raises(ValueError, match="unknown flag"):
        rep.keep(drop=("suspect", "wrong"))
    # ambiguous: by std_margin descending, ties by index; entries without a finite visit are left out
    std = rep.std_margin
    order = sorted((e for e in range(8) if rep.seen_finite[e] > 0), key=lambda e: (-std[e], e))
    assert rep.ambiguous(8).tolist() == order and rep.ambiguous(2).tolist() == order[:2] and order[0] == 0
    text = rep.report(worst=2)
    assert text.isascii() and text.startswith("clip ledger: 8 entries, 70021 rows in 19 updates") and "suspect" in text and "entry 5:" in text


def test_suspect_order_breaks_ties_by_index():
    rep = LedgerReport.from_arrays(5, seen=[2, 2, 2, 2, 0], sum_q=[-65536, -131072, -65536, 65536, 0], sum_q2=[1 << 32] * 4 + [0],
                                   min_q=[-65536] * 4 + [ref.INT32_MAX], max_q=[0] * 4 + [ref.INT32_MIN])
    assert rep.mean_margin[:4].tolist() == [-0.5, -1.0, -0.5, 0.5] and math.isnan(rep.mean_margin[4])
    assert rep.suspects().tolist() == [1, 0, 2] and rep.suspects(2).tolist() == [1, 0]
    assert rep.flags()["unseen"].tolist() == [False] * 4 + [True]
    with pytest.raises(ValueError):
        LedgerReport.from_arrays(2, margin=[1, 2])
    with pytest.raises(RuntimeError, match="overwritten"):
        LedgerReport.from_buffer(ref.RefLedger(3).tobytes()[:64 + 112], 2)
    with pytest.raises(ValueError, match="bytes"):
        LedgerReport.from_buffer(b"\0" * 100, 1)


def _random_rows(rng, n, n_entries):
    z = (rng.standard_normal((n, 2)) * 3).astype(np.float32)
    y = rng.integers(0, 2, n)
    e = rng.integers(-1, n_entries + 1, n)                                      # some skipped, some out of range
    y[rng.integers(0, n, 3)] = 2
    z[rng.integers(0, n, 2), 1] = np.nan
    return z, y, e


def test_sum_of_two_reports_is_the_report_of_the_concatenated_visits():
    rng = np.random.default_rng(5)
    a, b, both = ref.RefLedger(11), ref.RefLedger(11), ref.RefLedger(11)
    for k in range(6):
        z, y, e = _random_rows(rng, 40, 11)
        ep = [0, 1, 31, 32, 63, -1][k]
        (a if k % 2 == 0 else b).update(z, y, e, ep)
        both.update(z, y, e, ep)
    ra, rb = _report(a), _report(b)
    total = ra + rb
    assert total.tobytes() == both.tobytes() and total == _report(both) and (rb + ra) == total
    assert total.header["updates"] == 6 and total.header["rows"] == 240 and total.header["bad_labels"] > 0 and total.header["skipped"] > 0
    _check_against_visits(total, both)
    assert (ra + _report(ref.RefLedger(11))) == ra                              # a cleared ledger is the neutral element: min / max too
    with pytest.raises(ValueError, match="entries"):
        ra + _report(ref.RefLedger(10))


def test_epoch_counter_of_a_ledger_needs_no_device():
    """begin_epoch's bookkeeping alone: epochs 0..63, then -1 with ONE warning."""
    lg = led.ClipLedger.__new__(led.ClipLedger)
    lg._begun, lg._warned = 0, False
    assert lg.epoch == -1
    assert [lg.begin_epoch() for _ in range(64)] == list(range(64))
    with pytest.warns(RuntimeWarning, match="64 epochs"):
        assert lg.begin_epoch() == -1
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert lg.begin_epoch() == -1 and lg.epoch == -1                        # no second warning
    if not HAS_GPU:
        with pytest.raises(RuntimeError):
            led.ClipLedger(4, "cpu")


# ---- bank.loader(entries=...) ----------------------------------------------------------------------------------------------------
def test_loader_entries_argument_checks():
    b, _, _ = hb._mixed_bank()                                                  # 10 entries
    for bad, word in ((np.ones(9, bool), "mask of 9"), (np.zeros(10, bool), "empty"), ([], "empty"), ([0, 10], "outside"), ([-1, 2], "outside"),
                      ([3, 3], "strictly increasing"), ([4, 1], "strictly increasing"), ([0.5, 1.5], "mask"), (np.ones((2, 5), bool), "1-D")):
        with pytest.raises(ValueError, match=word):
            b.loader(4, entries=bad)
    assert b.loader(4).entries is None
    assert b.loader(4, entries=np.arange(10) % 2 == 0).entries.tolist() == [0, 2, 4, 6, 8] == b.select_entries([0, 2, 4, 6, 8]).tolist()


def test_loader_entries_restrict_len_order_and_batches_and_name_their_rows():
    import random
    b, _, seen = hb._mixed_bank()
    assert b.item_entries().tolist() == [0, 1, 2, 3, 4, 8, 9] + [5] * 11 + [6]
    ld = b.loader(4, entries=[1, 2, 5, 9])
    assert ld.item_entries().tolist() == [1, 2, 9] + [5] * 11 and len(ld) == 4 and ld.order() == list(range(14))
    assert len(b.loader(4, entries=[1, 2, 5, 9], drop_last=True)) == 3
    torch.manual_seed(3)
    want = torch.randperm(14).tolist()
    torch.manual_seed(3)
    assert b.loader(4, shuffle=True, entries=[1, 2, 5, 9]).order() == want
    torch.manual_seed(4)
    order = b.loader(4, shuffle=True, positive_fraction=0.5, entries=[1, 2, 5, 9]).order()
    picked = ld.item_entries()[order]
    assert len(order) == 14 and set(picked.tolist()) <= {1, 2, 5, 9} and int(b.labels[picked].sum()) == 7
    random.seed(2)
    assert ld.last_entries is None
    rows = []
    for data, target in ld:
        assert ld.last_entries.dtype == np.int64 and ld.last_entries.shape == (data.shape[0],)
        rows += ld.last_entries.tolist()
        entries = seen[-1][0]
        assert np.array_equal(ld.last_entries, np.where(b.ok[entries], entries, -1))               # bank coordinates; -1 for the placeholder
        assert target[:, 0].tolist() == b.labels[entries].tolist()
    assert rows == [1, -1, 9] + [5] * 11
    # entries=None is the loader it always was: the same gathers, the same draws
    del seen[:]
    random.seed(9)
    list(b.loader(4))
    first = [(e.tolist(), s.tolist()) for e, s, _ in seen]
    del seen[:]
    random.seed(9)
    list(b.loader(4, entries=None))
    assert first == [(e.tolist(), s.tolist()) for e, s, _ in seen]
    del seen[:]
    random.seed(9)
    list(b.loader(4, entries=np.ones(10, bool)))                                                    # and so is the full mask
    assert first == [(e.tolist(), s.tolist()) for e, s, _ in seen]
