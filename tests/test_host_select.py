"""Loss-ranked selection without a GPU: the float64 reference of tests/select_ref.py against torch and against the
restatements it sits beside, mining.HardSelect, the binding, and every refusal the library and the trainer make before they touch a device."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_ref
import mixup_ref
import select_ref as ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import ops

L = nat.lib
EINVAL = nat.WW_EINVAL


@pytest.mark.parametrize("name", list(ref.OPTION_SETS))
def test_per_clip_losses_match_torch_and_the_batch_restatement(name):
    o = ref.OPTION_SETS[name]
    z, y = ref.random_inputs(257, 3.0, seed=11)
    y[5::17] = -100                                                 # torch's default ignore_index; a bad label under the plain rule
    li, counting, cls = ref.losses(z, y, o)
    zt, w = torch.from_numpy(z).double(), None if "weight" not in o else torch.tensor(o["weight"], dtype=torch.float64)
    ignore = o.get("ignore_index", -100)
    yt = torch.from_numpy(loss_ref.torch_labels(y, ignore))
    if "focal_gamma" in o:                                          # Lin et al.: w_y (1 - p_y)^gamma (-log p_y)
        logp = F.log_softmax(zt, dim=1)
        ce = F.nll_loss(logp, yt, reduction="none", ignore_index=ignore)
        want = ((1.0 - torch.exp(-ce)) ** o["focal_gamma"] * ce).numpy()
        tol = 1e-9                                                  # 1 - p_y in place of the other class's term
    else:
        want = F.cross_entropy(zt, yt, weight=w, label_smoothing=o.get("label_smoothing", 0.0), ignore_index=ignore, reduction="none").numpy()
        tol = 1e-13
    assert np.abs(li - want).max() <= tol * max(1.0, np.abs(want).max())
    assert np.array_equal(counting, (y == 0) | (y == 1) if ignore != 1 else y == 0) and np.array_equal(cls[counting], y[counting])
    total = loss_ref.loss(z, y, o.get("weight") or (1.0, 1.0), o.get("label_smoothing", 0.0), ignore, "sum", o.get("focal_gamma"))["loss"]
    assert abs(li.sum() - total) <= 1e-12 * abs(total)


def test_the_plain_rule_and_probability_targets():
    z, y = ref.random_inputs(130, 3.0, seed=12)
    y[7] = -100
    li, counting, _ = ref.losses(z, y, None)                        # the plain rule: -100 is a bad label
    assert not counting[7] and li[7] == 0.0
    want = F.cross_entropy(torch.from_numpy(z).double()[counting], torch.from_numpy(y)[counting], reduction="none").numpy()
    assert np.abs(li[counting] - want).max() <= 1e-13 * max(1.0, want.max())
    zs, t = ref.random_inputs(130, 3.0, seed=13, soft=True)
    t[3] = (np.nan, 0.5); t[9] = (-0.25, 1.25)
    for o in ({}, {"weight": (1.0, 7.5)}, {"label_smoothing": 0.1}):
        li, counting, cls = ref.losses(zs, t, o)
        assert not counting[3] and not counting[9] and counting.sum() == 128
        w = None if "weight" not in o else torch.tensor(o["weight"], dtype=torch.float64)
        want = F.cross_entropy(torch.from_numpy(zs).double()[counting], torch.from_numpy(t).double()[counting], weight=w,
                               label_smoothing=o.get("label_smoothing", 0.0), reduction="none").numpy()
        assert np.abs(li[counting] - want).max() <= 1e-13 * max(1.0, want.max())
        total = mixup_ref.soft_loss(zs, t, o.get("weight") or (1.0, 1.0), o.get("label_smoothing", 0.0), "sum")["loss"]
        assert abs(li.sum() - total) <= 1e-12 * abs(total)
        assert np.array_equal(cls[counting], (t[counting, 1] > t[counting, 0]).astype(np.int64))


def test_reference_selection_is_topk_on_separated_losses():
    for n, keep in ((64, 1), (257, 40), (1025, 1025), (4097, 1000)):
        z, y, kind = ref.grid_inputs(n, seed=n)
        li, counting, cls = ref.losses(z, y, None)
        rank = ref.ranks(z, li, counting, cls)
        assert (rank == 1).all() and ref.min_gap(li, kind) >= 1e6 * ref.bound(z).max()
        sel = ref.select(ref.scores_of(li, rank), rank, keep)
        assert sel.size == keep and (np.diff(sel) > 0).all()
        # torch.topk breaks ties its own way: compare what cannot depend on that -- the multiset of kept losses and every row above the cut
        top = torch.topk(torch.from_numpy(li), keep).values.numpy()
        assert np.array_equal(np.sort(li[sel]), np.sort(top))
        assert set(np.flatnonzero(li > top.min())) <= set(sel.tolist())
        at = np.flatnonzero(li == top.min())                        # the tie group at the cut: its first rows by index
        assert np.array_equal(np.intersect1d(sel, at), at[:np.intersect1d(sel, at).size])


def test_reference_order_puts_the_kept_class_first_and_unranked_rows_last():
    z, y = ref.random_inputs(40, 1.0, seed=3)
    y[[4, 20]] = (-100, 7)
    z[11, 0] = np.nan; z[30, 1] = np.inf
    o = {"weight": (1.0, 2.0)}
    li, counting, cls = ref.losses(z, y, o)
    rank = ref.ranks(z, li, counting, cls, keep_class=1)
    assert list(np.flatnonzero(rank == 0)) == [4, 11, 20, 30] and set(np.flatnonzero(rank == 2)) == set(np.flatnonzero(y == 1)) - {11, 30}
    sc = ref.scores_of(li, rank)
    assert np.isneginf(sc[[4, 11, 20, 30]]).all()
    od = ref.order(sc, rank)
    n2 = int((rank == 2).sum())
    assert (rank[od[:n2]] == 2).all() and list(od[-4:]) == [4, 11, 20, 30] and (np.diff(sc[od[:n2]]) <= 0).all()
    assert np.array_equal(ref.select(sc, rank, 40), np.arange(40))
    s = ref.stats(sc, rank, counting, cls, ref.select(sc, rank, 38))
    assert s["kept_unranked"] == 2 and s["unranked"] == 4 and s["threshold"] == -np.inf and s["kept_positive"] == s["candidate_positive"]


def test_grid_inputs_stay_separated_under_the_options_the_gpu_test_uses():
    for n in (257, 4097, 65536):
        z, y, kind = ref.grid_inputs(n, seed=n)
        for o in (None, {"weight": (1.0, 7.5)}):
            li, _, _ = ref.losses(z, y, o)
            first = np.unique(kind, return_index=True)[1]
            assert np.array_equal(li, li[first][np.searchsorted(kind[first], kind)])         # copies of a row have one loss, bit for bit
            assert ref.min_gap(li, kind) >= 1e6 * ref.bound(z, (1.0, 7.5) if o else (1.0, 1.0)).max()


def test_hard_select_validates_at_construction():
    hs = pkg.HardSelect(0.25, keep_class=1)
    assert (hs.keep, hs.keep_class) == (0.25, 1) and hs.rows(4096) == 1024 and hs.rows(5) == 2 and hs.rows(1) == 1
    assert pkg.HardSelect(1.0).rows(7) == 7 and pkg.HardSelect(0.3).rows(10) == 3 and pkg.HardSelect(1e-9).rows(16) == 1
    assert pkg.HardSelect(5).rows(16) == 5 and pkg.HardSelect(5).rows(3) == 3 and pkg.HardSelect(np.int64(4)).keep == 4
    assert pkg.HardSelect(1, keep_class=0).keep_class == 0 and "keep_class=1" in repr(hs)
    for bad in (True, "0.5", None, [1]):
        with pytest.raises(TypeError):
            pkg.HardSelect(bad)
    for bad in (0, -3, 0.0, 1.5, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pkg.HardSelect(bad)
    for bad in (True, 1.0, "1"):
        with pytest.raises(TypeError):
            pkg.HardSelect(4, keep_class=bad)
    for bad in (2, -1):
        with pytest.raises(ValueError):
            pkg.HardSelect(4, keep_class=bad)
    with pytest.raises(ValueError):
        hs.rows(0)
    from wakeword_jupyterlab_amd import mining
    assert mining.HardSelect is pkg.HardSelect


def test_the_entries_are_bound_and_the_abi_stays_4():
    assert L.ww_abi_version() == nat.ABI_VERSION == 4
    assert nat.PROTOTYPES["ww_hard_select_workspace_bytes"] == (C.c_int64, [C.c_int64])
    assert nat.PROTOTYPES["ww_hard_select_f32"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.POINTER(nat.LossOpts), C.c_int32]
                                                    + [C.c_void_p] * 5)
    assert nat.PROTOTYPES["ww_select_rows_f32"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
                                                    + [C.c_void_p] * 6)
    for name in ("ww_hard_select_workspace_bytes", "ww_hard_select_f32", "ww_select_rows_f32"):
        fn = getattr(L, name)
        assert fn.argtypes == nat.PROTOTYPES[name][1] and fn.restype == nat.PROTOTYPES[name][0]
    assert C.sizeof(nat.SelectStats) == 64 == 8 * len(ops.SELECT_STATS_FIELDS)
    assert [f for f, _ in nat.SelectStats._fields_] == list(ops.SELECT_STATS_FIELDS)
    assert L.ww_hard_select_workspace_bytes(1) == 512 and L.ww_hard_select_workspace_bytes(65536) == 65536 * 9
    assert L.ww_hard_select_workspace_bytes(257) == 2304 + 512
    assert L.ww_hard_select_workspace_bytes(0) == EINVAL and L.ww_hard_select_workspace_bytes(65537) == EINVAL


def _select(logits=256, targets=512, kind=0, n=8, keep=4, opts=None, keep_class=-1, sel=768, scores=None, stats=None, ws=1024):
    return L.ww_hard_select_f32(logits, targets, kind, n, keep, None if opts is None else C.byref(opts), keep_class, sel, scores, stats, ws, None)


@pytest.mark.parametrize("kw, word", [
    (dict(n=65537, keep=4), "n 65537"), (dict(n=0, keep=1), "n 0"), (dict(keep=0), "keep 0"), (dict(keep=-1), "keep -1"), (dict(keep=9), "keep 9"),
    (dict(keep_class=2), "keep_class 2"), (dict(keep_class=-2), "keep_class -2"), (dict(kind=2), "target_kind 2"), (dict(kind=-1), "target_kind"),
    (dict(logits=None), "null"), (dict(targets=None), "null"), (dict(sel=None), "null"), (dict(ws=None), "null"),
    (dict(logits=258), "4-byte"), (dict(targets=516), "8-byte"), (dict(kind=1, targets=514), "4-byte"), (dict(sel=772), "8-byte"),
    (dict(scores=12), "8-byte"), (dict(stats=20), "8-byte"), (dict(ws=1032), "256-byte"),
])
def test_hard_select_refuses_bad_arguments_before_any_hip_call(kw, word):
    assert _select(**kw) == EINVAL
    assert word in L.ww_last_error().decode()


def test_hard_select_checks_the_options_as_the_loss_entries_do():
    for change, word in ((dict(label_smoothing=1.5), "label_smoothing"), (dict(focal_gamma=-1.0), "focal_gamma"), (dict(kind=7), "kind")):
        o = ops.loss_opts(weight=(1.0, 2.0))
        for k, v in change.items():
            setattr(o, k, v)
        assert _select(opts=o) == EINVAL and word in L.ww_last_error().decode()
    o = ops.loss_opts(weight=(1.0, 2.0)); o.class_weight[1] = -1.0
    assert _select(opts=o) == EINVAL and "class_weight" in L.ww_last_error().decode()
    assert _select(kind=1, opts=ops.loss_opts(focal_gamma=2.0)) == EINVAL and "WW_LOSS_CE" in L.ww_last_error().decode()
    assert _select(kind=1, opts=ops.loss_opts(ignore_index=1)) == EINVAL and "ignore_index" in L.ww_last_error().decode()
    if not torch.cuda.is_available():                               # good arguments: only the device is missing
        assert _select(opts=ops.loss_opts(weight=(1.0, 2.0)), keep_class=1, scores=2048, stats=4096) == nat.WW_ENODEVICE


def _rows(mel=4096, n=8, width=32, sel=256, keep=4, mel_out=1 << 20, targets=None, kind=0, targets_out=None, entries=None, entries_out=None,
          labels=None, labels_out=None):
    return L.ww_select_rows_f32(mel, n, width, sel, keep, mel_out, targets, kind, targets_out, entries, entries_out, labels, labels_out, None)


@pytest.mark.parametrize("kw, code, word", [
    (dict(n=0), EINVAL, "n 0"), (dict(keep=0), EINVAL, "keep 0"), (dict(keep=9), EINVAL, "keep 9"), (dict(width=0), nat.WW_EUNSUPPORTED, "width 0"),
    (dict(width=33), nat.WW_EUNSUPPORTED, "width 33"), (dict(sel=None), EINVAL, "sel"), (dict(mel_out=None), EINVAL, "both"),
    (dict(targets=512), EINVAL, "both"), (dict(entries_out=512), EINVAL, "both"), (dict(mel=None, mel_out=None), EINVAL, "nothing"),
    (dict(targets=1 << 21, targets_out=1 << 22, kind=5), EINVAL, "target_kind"), (dict(mel=4098), EINVAL, "4-byte"), (dict(sel=260), EINVAL, "8-byte"),
    (dict(targets=(1 << 21) + 4, targets_out=1 << 22), EINVAL, "8-byte"), (dict(labels=1 << 21, labels_out=(1 << 22) + 4), EINVAL, "8-byte"),
    (dict(mel_out=4096 + 80 * 32 * 4 * 7), EINVAL, "overlaps"), (dict(entries=1 << 21, entries_out=(1 << 21) + 8), EINVAL, "overlaps"),
])
def test_select_rows_refuses_bad_arguments_before_any_hip_call(kw, code, word):
    assert _rows(**kw) == code
    assert word in L.ww_last_error().decode()


def test_ops_and_stats_helpers_without_a_device():
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        ops.new_select_stats("cpu")
    host = torch.tensor([3, 300, 75, 40, 30, 2, 0, 0], dtype=torch.int64)
    host[7:].view(torch.float64)[0] = 0.625
    assert ops.read_select_stats(host) == {"batches": 3, "candidates": 300, "kept": 75, "candidate_positive": 40, "kept_positive": 30,
                                           "unranked": 2, "kept_unranked": 0, "threshold": 0.625}
    fresh = ops.read_select_stats(torch.zeros(8, dtype=torch.int64))
    assert fresh["batches"] == 0 and fresh["threshold"] != fresh["threshold"]
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        ops.hard_select(torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64), 2)
    assert ops.hard_select_workspace_bytes(4096) == 4096 * 9
    with pytest.raises(nat.NativeError):
        ops.hard_select_workspace_bytes(1 << 17)
    for bad in (2, -1, True, 1.0):
        with pytest.raises(ValueError):
            ops._keep_class(bad)
    from wakeword_jupyterlab_amd.trainer import WakewordTrainer
    r = WakewordTrainer._select_report({"batches": 2, "candidates": 200, "kept": 50, "candidate_positive": 20, "kept_positive": 15, "unranked": 1,
                                        "kept_unranked": 0, "threshold": 0.5})
    assert (r["kept_fraction"], r["candidate_positive_fraction"], r["kept_positive_fraction"], r["threshold"]) == (0.25, 0.1, 0.3, 0.5)
    empty = WakewordTrainer._select_report(ops.read_select_stats(torch.zeros(8, dtype=torch.int64)))
    assert empty["kept_fraction"] != empty["kept_fraction"] and empty["batches"] == 0


def test_trainer_refusals_without_a_device():
    student, teacher = pkg.SimpleWakewordModel(), pkg.WakewordModel().eval()
    with pytest.raises(NotImplementedError, match="select"):
        pkg.WakewordTrainer(student, "cpu", teacher=teacher, select=pkg.HardSelect(4))
    with pytest.raises(TypeError, match="HardSelect"):
        pkg.WakewordTrainer(student, "cpu", select=0.25)
    with pytest.raises(TypeError, match="CPU"):                     # a good rule: the next refusal is the old one
        pkg.WakewordTrainer(student, "cpu", select=pkg.HardSelect(4))
    from wakeword_jupyterlab_amd.trainer import WakewordTrainer
    with pytest.raises(NotImplementedError):
        WakewordTrainer._check_select(pkg.HardSelect(0.5), teacher)
    assert WakewordTrainer._check_select(None, teacher) is None and WakewordTrainer._check_select(pkg.HardSelect(0.5), None) is None
