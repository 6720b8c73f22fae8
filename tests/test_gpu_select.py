"""Loss-ranked selection on the GPU (csrc/ww_select.hip): the scores against the float64 reference of
tests/select_ref.py, the selection against the three-key order applied on the host to the scores the kernel emitted (no tolerance), ties,
rank classes and the stats record, memory contracts, the row gather, and WakewordTrainer's `select=` against a twin driven by hand.

The score bound is derived, not measured: lse - z_y cancels, so a score may be off by 2^-46 max(1, |z0|, |z1|) (w0 + w1) -- about 64
float64 ulps of the largest intermediate (select_ref.bound)."""
import ctypes as C

import numpy as np
import pytest
import torch

import select_ref as ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import ops
from ws_harness import Guarded

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
L = nat.lib


def _opts(targets, kw):
    """The options struct for a kind of target; None stays None (the plain rule / the soft defaults)."""
    if kw is None:
        return None
    return ops.soft_loss_opts(**kw) if np.asarray(targets).dtype.kind == "f" else ops.loss_opts(**kw)


def _run(z, t, keep, kw=None, keep_class=None):
    """One ww_hard_select_f32 call through ops.hard_select_into with a stats record: (sel, scores, stats dict) on the host."""
    n = z.shape[0]
    zd, td = torch.from_numpy(z).to(DEV), torch.from_numpy(t).to(DEV)
    sel = torch.full((keep,), -7, device=DEV, dtype=torch.int64)
    scores = torch.full((n,), 123.0, device=DEV, dtype=torch.float64)
    stats = ops.new_select_stats(DEV)
    ws = torch.empty(ops.hard_select_workspace_bytes(n), device=DEV, dtype=torch.uint8)
    ops.hard_select_into(zd, td, keep, sel, scores, stats, ws, opts=_opts(t, kw), keep_class=keep_class)
    return sel.cpu().numpy(), scores.cpu().numpy(), ops.read_select_stats(stats)


def _check_against_emitted(z, t, kw, keep_class, keep, sel, scores, stats=None):
    """sel is EXACTLY the first `keep` rows of the order over the emitted scores; the record matches; returns the reference pieces."""
    li, counting, cls = ref.losses(z, t, kw)
    rank = ref.ranks(z, scores, counting, cls, keep_class)           # the rank's "finite score" is the emitted one's
    assert np.array_equal(rank, ref.ranks(z, li, counting, cls, keep_class))
    assert np.isneginf(scores[rank == 0]).all() and np.isfinite(scores[rank > 0]).all()
    want = ref.select(scores, rank, keep)
    assert sel.shape == (keep,) and (np.diff(sel) > 0).all() and np.array_equal(sel, want), (sel[:8], want[:8])
    if stats is not None:
        assert stats == ref.stats(scores, rank, counting, cls, sel)
    return li, rank


def _plant_unranked(z, t):
    """Rows no criterion ranks, where the batch has room: a NaN and an Inf logit, a label 7 / an invalid probability row."""
    n = z.shape[0]
    if n >= 8:
        z[n // 3, 0] = np.nan
        z[n // 2, 1] = np.inf
        if t.dtype.kind == "f":
            t[n // 5] = (np.nan, 0.5)
            t[n // 7] = (-0.5, 1.5)
        else:
            t[n // 5] = 7
            t[n // 7] = -100
    return z, t


# ---- scores ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.SIZES)
def test_scores_match_the_float64_reference(n):
    worst = 0.0
    for scale in (1.0, 30.0):
        cases = [(False, name, kw) for name, kw in ref.OPTION_SETS.items()] + [(False, "plain", None)]
        cases += [(True, name, ref.OPTION_SETS[name]) for name in ("default", "weights", "smoothing")] + [(True, "null", None)]
        for soft, name, kw in cases:
            z, t = _plant_unranked(*ref.random_inputs(n, scale, seed=7 * n + int(scale), soft=soft))
            keep = max(1, n // 2)
            sel, scores, stats = _run(z, t, keep, kw)
            li, rank = _check_against_emitted(z, t, kw, None, keep, sel, scores, stats)
            if name == "ignore":
                assert (rank[t == 1] == 0).all()                    # ignore_index = 1 hits every positive
            err = np.abs(scores[rank > 0] - li[rank > 0]) / ref.bound(z, (kw or {}).get("weight") or (1.0, 1.0))[rank > 0]
            if err.size:
                worst = max(worst, float(err.max()))
            assert (err <= 1.0).all(), f"n={n} scale={scale} soft={soft} {name}: {err.max():.3f} x the bound"
    print(f"n={n}: worst score error {worst:.4f} x the bound")


# ---- selection ---------------------------------------------------------------------------------------------------------------------------
def _keeps(n):
    return sorted({k for k in (1, 2, n // 2, n - 1, n) if 1 <= k <= n})


@pytest.mark.parametrize("n", ref.SIZES)
def test_selection_is_the_three_key_order_of_the_emitted_scores(n):
    for soft, kw, keep_class in ((False, None, None), (False, {"weight": (1.0, 7.5)}, 1), (True, None, 0)):
        z, t = _plant_unranked(*ref.random_inputs(n, 1.0, seed=13 * n + 1, soft=soft))
        for keep in _keeps(n):
            sel, scores, stats = _run(z, t, keep, kw, keep_class)
            _check_against_emitted(z, t, kw, keep_class, keep, sel, scores, stats)
            if keep == n:
                assert np.array_equal(sel, np.arange(n))


@pytest.mark.parametrize("n", (257, 4097, 65536))
def test_selection_on_separated_losses_is_the_references_own(n):
    z, y, kind = ref.grid_inputs(n, seed=n)
    for kw, keep_class in ((None, None), ({"weight": (1.0, 7.5)}, None), (None, 1)):
        li, counting, cls = ref.losses(z, y, kw)
        assert ref.min_gap(li, kind) >= 1e6 * ref.bound(z, (1.0, 7.5) if kw else (1.0, 1.0)).max()      # confirmed on the CPU
        rank = ref.ranks(z, li, counting, cls, keep_class)
        for keep in _keeps(n):
            sel, scores, _ = _run(z, y, keep, kw, keep_class)
            assert np.array_equal(sel, ref.select(ref.scores_of(li, rank), rank, keep)), f"n={n} keep={keep} {kw} {keep_class}"


# ---- ties --------------------------------------------------------------------------------------------------------------------------------
def test_identical_rows_are_taken_in_index_order():
    for n in (5, 1025, 4097):
        z = np.tile(np.array([[0.25, -1.5]], np.float32), (n, 1))
        y = np.ones(n, np.int64)
        for keep in _keeps(n) + [min(n, 700)]:
            sel, scores, stats = _run(z, y, keep)
            assert np.array_equal(sel, np.arange(keep)) and np.unique(scores).size == 1
            assert stats["threshold"] == scores[0] and stats["kept_positive"] == keep


def test_a_tie_group_cut_by_keep():
    n = 2049
    copies, hard = [0, 63, 64, 255, 256, 1023, 1024, n - 1], [10, 11, 12, 500, 2000]
    z = np.tile(np.array([[0.0, 5.0]], np.float32), (n, 1))          # easy rows, themselves one tie group
    z[copies] = (0.0, -2.0)
    z[hard] = (0.0, -6.0)
    y = np.ones(n, np.int64)
    for keep, want in ((3, hard[:3]), (5 + 3, hard + copies[:3]), (5 + 7, hard + copies[:7]), (5 + 8, hard + copies),
                       (5 + 8 + 2, hard + copies + [1, 2])):
        sel, scores, stats = _run(z, y, keep)
        assert np.array_equal(sel, np.sort(np.array(want))), (keep, sel)
        _check_against_emitted(z, y, None, None, keep, sel, scores, stats)


# ---- rank classes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", (False, True))
def test_rank_classes_and_the_stats_record(soft):
    n = 300
    kw = {"weight": (1.0, 2.0)} if soft else {"weight": (1.0, 2.0), "ignore_index": -100}
    for positives in (40, 7, 0):                                     # more, fewer and no positives than / of the rows kept
        rng = np.random.default_rng(50 + positives)
        z = rng.standard_normal((n, 2)).astype(np.float32)
        pos = rng.permutation(n)[:positives]
        if soft:
            t = np.tile(np.array([[0.9, 0.1]], np.float32), (n, 1))
            t[pos] = (0.2, 0.8)
            t[[17, 130]] = [(np.nan, 1.0), (0.5, -0.5)]
        else:
            t = np.zeros(n, np.int64)
            t[pos] = 1
            t[[17, 130]] = (-100, 7)                                 # ignored, bad
        z[[44, 250], [0, 1]] = (np.nan, -np.inf)
        unranked = [17, 44, 130, 250]
        for keep in (20, n - len(unranked), n - len(unranked) + 2, n):
            sel, scores, stats = _run(z, t, keep, kw, keep_class=1)
            li, rank = _check_against_emitted(z, t, kw, 1, keep, sel, scores, stats)
            assert list(np.flatnonzero(rank == 0)) == unranked and stats["unranked"] == 4
            ranked_pos = np.flatnonzero(rank == 2)
            assert len(np.intersect1d(sel, ranked_pos)) == min(keep, ranked_pos.size)        # the kept class goes first
            chosen_unranked = [i for i in unranked if i in set(sel.tolist())]
            assert chosen_unranked == unranked[:max(0, keep - (n - 4))]                      # last, in index order, only when nothing is left
            assert stats["kept_unranked"] == len(chosen_unranked)
            assert (stats["threshold"] == -np.inf) == (len(chosen_unranked) > 0)


# ---- memory and repeatability ------------------------------------------------------------------------------------------------------------
def test_offset_views_guard_bands_and_repeatability():
    n, keep = 1025, 300
    z, y = _plant_unranked(*ref.random_inputs(n, 3.0, seed=5))
    zs, t = _plant_unranked(*ref.random_inputs(n, 3.0, seed=6, soft=True))
    o = ops.loss_opts(weight=(1.0, 7.5))
    for soft, logits, targets in ((False, z, y), (True, zs, t)):
        base_sel, base_scores, base_stats = _run(logits, targets, keep, {"weight": (1.0, 7.5)}, 1)
        # views offset by one element: logits and probabilities 4 bytes off the 16-byte grid, labels 8 bytes off it
        zbuf = torch.zeros(2 * n + 1, device=DEV, dtype=torch.float32)
        zbuf[1:] = torch.from_numpy(logits).reshape(-1).to(DEV)
        tflat = torch.from_numpy(targets).reshape(-1).to(DEV)
        tbuf = torch.zeros(tflat.numel() + 1, device=DEV, dtype=tflat.dtype)
        tbuf[1:] = tflat
        zv, tv = zbuf[1:].view(n, 2), tbuf[1:].view(n, 2) if soft else tbuf[1:]
        assert zv.data_ptr() % 16 == 4 and tv.data_ptr() % 16 == (4 if soft else 8)
        results = []
        for fill in (0x00, 0xFF, 0xFF):                              # the workspace's content does not matter; two launches, the same bytes
            ws = Guarded(ops.hard_select_workspace_bytes(n), fill, device=DEV)
            gsel = Guarded.for_output((keep,), torch.int64, device=DEV)
            gsc = Guarded.for_output((n,), torch.float64, device=DEV)
            gst = Guarded.for_output((8,), torch.int64, device=DEV, fill=0)
            rc = L.ww_hard_select_f32(zv.data_ptr(), tv.data_ptr(), int(soft), n, keep, C.byref(o), 1, gsel.ptr, gsc.ptr, gst.ptr, ws.ptr,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, L.ww_last_error()
            torch.cuda.synchronize()
            assert ws.intact() and gsel.intact() and gsc.intact() and gst.intact()
            results.append((gsel.bytes().cpu(), gsc.bytes().cpu(), gst.bytes().cpu()))
        for other in results[1:]:
            assert all(torch.equal(a, b) for a, b in zip(results[0], other))
        assert np.array_equal(results[0][0].numpy().view(np.int64), base_sel)
        assert np.array_equal(results[0][1].numpy().view(np.float64), base_scores)
        assert ops.read_select_stats(results[0][2].view(torch.int64)) == base_stats
        assert np.array_equal(zbuf[1:].cpu().numpy().view(np.int32), logits.reshape(-1).view(np.int32)) and zbuf[0] == 0 and tbuf[0] == 0
        assert np.array_equal(tbuf[1:].cpu().numpy().view(np.uint8), targets.reshape(-1).view(np.uint8))                # inputs untouched


def test_null_scores_and_stats_and_the_allocating_form():
    z, y = ref.random_inputs(257, 2.0, seed=9)
    zd, yd = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
    sel, scores = ops.hard_select(zd, yd[:, None], 31, opts=ops.loss_opts(focal_gamma=2.0), keep_class=1)
    base_sel, base_scores, _ = _run(z, y, 31, {"focal_gamma": 2.0}, 1)
    assert np.array_equal(sel.cpu().numpy(), base_sel) and np.array_equal(scores.cpu().numpy(), base_scores)
    sel2 = torch.empty(31, device=DEV, dtype=torch.int64)
    ws = torch.empty(ops.hard_select_workspace_bytes(257), device=DEV, dtype=torch.uint8)
    ops.hard_select_into(zd, yd, 31, sel2, None, None, ws, opts=ops.loss_opts(focal_gamma=2.0), keep_class=1)
    assert torch.equal(sel2, sel)
    with pytest.raises(ValueError):
        ops.hard_select(zd, yd, 258)
    with pytest.raises(ValueError):
        ops.hard_select(zd, yd, 0)


# ---- the gather ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", (8, 31, 32))
def test_select_rows_copies_the_selected_rows_bit_for_bit(T):
    n = 5
    g = torch.Generator().manual_seed(T)
    x = torch.randn(n, 1, 80, T, generator=g).to(DEV)
    y = torch.randint(0, 2, (n,), generator=g).to(DEV)
    t = torch.rand(n, 2, generator=g).to(DEV)
    entries = torch.randint(0, 1000, (n,), generator=g).to(DEV)
    labels = torch.randint(0, 2, (n,), generator=g).to(DEV)
    for rows in ([3], [0, 2, 4], [0, 1, 2, 3, 4], [4, 4, 1]):
        sel = torch.tensor(rows, device=DEV, dtype=torch.int64)
        k = len(rows)
        for targets in (y, t, None):
            for with_rest in (True, False):
                gx = Guarded.for_output((k, 1, 80, T), torch.float32, device=DEV)
                gt = None if targets is None else Guarded.for_output((k,) + tuple(targets.shape[1:]), targets.dtype, device=DEV)
                ge, gl = (Guarded.for_output((k,), torch.int64, device=DEV) for _ in range(2)) if with_rest else (None, None)
                ops.select_rows_into(x, sel, gx.view(), targets, None if gt is None else gt.view(), entries if with_rest else None,
                                     None if ge is None else ge.view(), labels if with_rest else None, None if gl is None else gl.view())
                torch.cuda.synchronize()
                assert all(b.intact() for b in (gx, gt, ge, gl) if b is not None)
                assert torch.equal(gx.view(), x[sel])
                assert gt is None or torch.equal(gt.view(), targets[sel])
                assert not with_rest or (torch.equal(ge.view(), entries[sel]) and torch.equal(gl.view(), labels[sel]))
    # off the 16-byte grid (one float at a time), and indices outside [0, n): rows of zeros, nothing read
    buf = torch.zeros(x.numel() + 1, device=DEV)
    buf[1:] = x.reshape(-1)
    xv = buf[1:].view(n, 1, 80, T)
    obuf = torch.full((3 * 80 * T + 2,), -9.0, device=DEV)
    out = obuf[1:-1].view(3, 1, 80, T)
    sel = torch.tensor([2, -1, n], device=DEV, dtype=torch.int64)
    yo = torch.full((3,), -5, device=DEV, dtype=torch.int64)
    ops.select_rows_into(xv, sel, out, y, yo)
    assert torch.equal(out[0], x[2]) and not out[1:].any() and obuf[0] == -9.0 and obuf[-1] == -9.0
    assert yo.tolist() == [int(y[2]), 0, 0]
    to = torch.full((3, 2), -5.0, device=DEV)
    ops.select_rows_into(x, sel, torch.empty(3, 1, 80, T, device=DEV), t, to)
    assert torch.equal(to[0], t[2]) and not to[1:].any()


# ---- the trainer -------------------------------------------------------------------------------------------------------------------------
MODELS = {"simple": pkg.SimpleWakewordModel, "full": pkg.WakewordModel}


def _batch(n, T, seed):
    g = torch.Generator().manual_seed(seed)
    x = (-40.0 + 20.0 * torch.randn(n, 1, 80, T, generator=g)).to(DEV)
    y = torch.randint(0, 2, (n,), generator=g).to(DEV)
    return x, y


def _trainer(name, **kw):
    torch.manual_seed(1234)                                          # fresh for each trainer: the weights, then the steps' dropout seeds
    model = MODELS[name]().to(DEV)
    model.train()
    return pkg.WakewordTrainer(model, DEV, **kw)


def _weights(trainer):
    return [p.detach().clone() for p in trainer.model.parameters()]


def test_keep_of_the_whole_batch_is_the_plain_step():
    x, y = _batch(16, 32, seed=1)
    plain, whole = _trainer("simple"), None
    for _ in range(3):
        plain.step(x, y)
    w_plain, loss_plain = _weights(plain), plain.last_loss.clone()
    for rule in (pkg.HardSelect(16), pkg.HardSelect(1.0), pkg.HardSelect(99)):
        whole = _trainer("simple", select=rule)
        for _ in range(3):
            whole.step(x, y)
        assert all(torch.equal(a, b) for a, b in zip(w_plain, _weights(whole))) and torch.equal(loss_plain, whole.last_loss)
        assert whole.last_selected is None and ops.read_select_stats(whole.select_stats)["batches"] == 0


@pytest.mark.parametrize("name, B, k", [("simple", 16, 5), ("simple", 64, 16), ("full", 8, 3)])
def test_mined_step_equals_a_twin_driven_by_hand(name, B, k):
    x, y = _batch(B, 32, seed=B + k)
    mined = _trainer(name, select=pkg.HardSelect(k))
    chosen = []
    for _ in range(3):
        mined.step(x, y)
        chosen.append(mined.last_selected.cpu().numpy().copy())
        assert mined.last_logits[:k].shape == (k, 2) and mined.last_scores.shape == (B,)
    w_mined, loss_mined = _weights(mined), mined.last_loss.clone()

    twin = _trainer(name)
    math = nat.lib.ww_get_train_math()
    ws = torch.empty(ops.train_workspace_bytes(B, twin._n_conv, math), device=DEV, dtype=torch.uint8)
    slogits = torch.empty(B, 2, device=DEV)
    for step in range(3):
        ops.train_forward_into(x, twin._tp, 0.0, 0.0, 0, math, ws, slogits)          # the scoring forward: dropout 0, no seed drawn
        _, scores = ops.hard_select(slogits, y, k)
        scores = scores.cpu().numpy()
        li, counting, cls = ref.losses(slogits.cpu().numpy(), y.cpu().numpy(), None)
        sel = ref.select(scores, ref.ranks(slogits.cpu().numpy(), scores, counting, cls), k)
        assert np.array_equal(sel, chosen[step])
        idx = torch.from_numpy(sel).to(DEV)
        twin.step(x[idx].contiguous(), y[idx].contiguous())
    assert all(torch.equal(a, b) for a, b in zip(w_mined, _weights(twin)))
    assert torch.equal(loss_mined.view(torch.int32), twin.last_loss.view(torch.int32))


def test_ledger_receives_the_kept_rows_under_their_entries():
    B, k = 16, 5
    x, y = _batch(B, 32, seed=3)
    for device_entries in (False, True):
        ledger = pkg.ClipLedger(100, DEV)
        trainer = _trainer("simple", select=pkg.HardSelect(k), ledger=ledger)
        entries = (np.arange(B, dtype=np.int64) * 7 + 3) % 100
        seen = np.zeros(100, np.int64)
        ledger.begin_epoch()
        for _ in range(3):
            trainer.step(x, y, entries=torch.from_numpy(entries).to(DEV) if device_entries else entries)
            seen[entries[trainer.last_selected.cpu().numpy()]] += 1
        report = ledger.read()
        assert report.header["rows"] == 3 * k and np.array_equal(report.seen, seen) and report.header["bad_entries"] == 0
        assert ops.read_loss_stats(trainer.train_stats)["total"] == 3 * k


def test_float_targets_are_gathered_with_their_rows():
    B, k = 16, 6
    x, y = _batch(B, 32, seed=4)
    g = torch.Generator().manual_seed(4)
    lam = torch.rand(B, generator=g).to(DEV)
    t = torch.stack([1.0 - lam, lam], dim=1).contiguous()
    ledger = pkg.ClipLedger(B, DEV)
    trainer = _trainer("simple", select=pkg.HardSelect(k, keep_class=1), ledger=ledger)
    ledger.begin_epoch()
    trainer.step(x, t, entries=np.arange(B), labels=y)
    sel = trainer.last_selected
    assert torch.equal(trainer._gathered["soft"], t[sel]) and torch.equal(trainer._gathered["x"], x[sel])
    assert torch.equal(trainer._gathered["labels"], y[sel]) and torch.equal(trainer._gathered["entries"], sel)
    scores = trainer.last_scores.cpu().numpy()
    li, counting, cls = ref.losses(trainer._slogits[:B].cpu().numpy(), t.cpu().numpy(), None)
    assert np.array_equal(sel.cpu().numpy(), ref.select(scores, ref.ranks(trainer._slogits[:B].cpu().numpy(), scores, counting, cls, 1), k))
    assert np.array_equal(np.flatnonzero(ledger.read().seen), np.sort(sel.cpu().numpy()))


def test_select_report_is_consistent_with_the_steps():
    B, k = 16, 4
    x, y = _batch(B, 32, seed=8)
    trainer = _trainer("simple", select=pkg.HardSelect(0.25, keep_class=1))
    assert trainer.select.rows(B) == k
    kept_positive, threshold = 0, None
    for _ in range(3):
        trainer.step(x, y)
        sel = trainer.last_selected
        kept_positive += int(y[sel].sum())
        threshold = float(trainer.last_scores[sel].min())
    s = ops.read_select_stats(trainer.select_stats)
    assert s == {"batches": 3, "candidates": 3 * B, "kept": 3 * k, "candidate_positive": 3 * int(y.sum()), "kept_positive": kept_positive,
                 "unranked": 0, "kept_unranked": 0, "threshold": threshold}
    loss, acc = trainer.train_epoch([(x, y)] * 2)                    # zeroes both records, reads them in one copy
    r = trainer.select_report
    assert (r["batches"], r["candidates"], r["kept"], r["kept_fraction"]) == (2, 2 * B, 2 * k, 0.25)
    assert r["candidate_positive_fraction"] == float(y.sum()) / B and r["unranked"] == 0
    assert r["threshold"] == float(trainer.last_scores[trainer.last_selected].min())
    assert np.isfinite(loss) and 0.0 <= acc <= 100.0 and ops.read_loss_stats(trainer.train_stats)["total"] == 2 * k
    trainer.select = None                                            # assignable; the plain step again
    trainer.step(x, y)
    assert ops.read_loss_stats(trainer.train_stats)["total"] == 2 * k + B
    with pytest.raises(TypeError):
        trainer.select = 0.5


def test_mined_step_has_no_hidden_waits_and_allocates_nothing():
    B = 16
    x, y = _batch(B, 8, seed=6)
    trainer = _trainer("simple", select=pkg.HardSelect(5, keep_class=1))
    for _ in range(2):
        trainer.step(x, y)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        trainer.step(x, y)
        trainer.step(x, y)
        before = torch.cuda.memory_allocated()
        trainer.step(x, y)
        after = torch.cuda.memory_allocated()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert before == after
    torch.cuda.synchronize()
    assert ops.read_loss_stats(trainer.train_stats)["batches"] == 5 and ops.read_select_stats(trainer.select_stats)["batches"] == 5


def test_mined_steps_of_changing_batch_size_allocate_nothing():
    """An epoch's ragged last batch and the full batch after it: the gather buffers only grow, like the logits' -- a step at a batch
    size that has been seen allocates nothing, whatever size came between."""
    trainer = _trainer("simple", select=pkg.HardSelect(0.5), ledger=pkg.ClipLedger(40, DEV))
    batches = {B: _batch(B, 8, seed=B) + (torch.arange(B, device=DEV),) for B in (16, 5)}
    for B in (16, 5):
        trainer.step(*batches[B][:2], entries=batches[B][2])
    torch.cuda.synchronize()
    import gc
    gc.collect()                                                     # earlier tests' trainers are not freed inside the window
    torch.cuda.set_sync_debug_mode("error")
    try:
        for B in (16, 5, 16):
            x, y, entries = batches[B]
            before = torch.cuda.memory_allocated()
            trainer.step(x, y, entries=entries)
            assert torch.cuda.memory_allocated() == before, B
            k = trainer.select.rows(B)
            assert trainer.last_selected.shape == (k,) and trainer.last_logits[:k].shape == (k, 2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    sel = trainer.last_selected
    assert torch.equal(trainer._gathered["x"][:8], batches[16][0][sel]) and torch.equal(trainer._gathered["entries"][:8], sel)
    assert ops.read_select_stats(trainer.select_stats)["batches"] == 5
