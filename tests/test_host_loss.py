"""The loss for imbalanced data without a GPU: every refused argument of ops.ce_loss, FocalLoss and the C
entry (before any HIP call, naming the field); FocalLoss.forward against float64 autograd; balanced_class_weights; the class-balanced
epoch order; and the float64 restatement of tests/loss_ref.py against torch on the CPU within the caps the GPU tests hold torch to."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import loss_ref as ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import ops
from wakeword_jupyterlab_amd.bank import BankLoader
from wakeword_jupyterlab_amd.dataset import GpuBatchLoader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = nat.lib
U = ref.U


def _err():
    return (L.ww_last_error() or b"").decode()


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------
def test_abi_stays_4_and_the_entry_and_struct_are_the_headers():
    assert L.ww_abi_version() == 4 == nat.ABI_VERSION
    assert nat.PROTOTYPES["ww_ce_loss_ex_f32"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(nat.LossOpts)] + [C.c_void_p] * 4)
    assert L.ww_ce_loss_ex_f32.argtypes == nat.PROTOTYPES["ww_ce_loss_ex_f32"][1]
    text = open(os.path.join(ROOT, "include", "wakeword_amd.h")).read()
    body = re.search(r"typedef struct ww_loss_opts \{(.*?)\} ww_loss_opts;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(double|int64_t|int32_t)\s+(\w+)(\[2\])?\s*;", body)
    ctype = {"double": C.c_double, "int64_t": C.c_int64, "int32_t": C.c_int32}
    assert [n for _, n, _ in fields] == [n for n, _ in nat.LossOpts._fields_]
    for (t, n, arr), (_, ct) in zip(fields, nat.LossOpts._fields_):
        assert ct is ctype[t] or (arr and ct._type_ is ctype[t] and ct._length_ == 2), n
    assert C.sizeof(nat.LossOpts) == 48 and nat.LossOpts.ignore_index.offset == 32 and nat.LossOpts.reduction.offset == 44
    for name, value in (("WW_LOSS_CE", nat.LOSS_CE), ("WW_LOSS_FOCAL", nat.LOSS_FOCAL), ("WW_REDUCE_MEAN", nat.REDUCE_MEAN),
                        ("WW_REDUCE_SUM", nat.REDUCE_SUM)):
        assert re.search(rf"#define {name} {value}\b", text)
    assert C.sizeof(nat.LossStats) == 48                                           # the record keeps its size


def _opts(**kw):
    o = nat.LossOpts()
    o.class_weight[0], o.class_weight[1] = kw.pop("w", (0.25, 4.0))
    o.label_smoothing, o.focal_gamma, o.ignore_index, o.kind, o.reduction = 0.0, 0.0, -100, nat.LOSS_CE, nat.REDUCE_MEAN
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _ex(opts, logits=16, labels=16, n=4, dlogits=None, loss=None, stats=None):
    return L.ww_ce_loss_ex_f32(logits, labels, n, None if opts is None else C.byref(opts), dlogits, loss, stats, None)


@pytest.mark.parametrize("kw, word", [
    (dict(w=(-1.0, 1.0)), "class_weight[0]"), (dict(w=(1.0, float("nan"))), "class_weight[1]"), (dict(w=(float("inf"), 1.0)), "class_weight[0]"),
    (dict(label_smoothing=-0.1), "label_smoothing"), (dict(label_smoothing=1.5), "label_smoothing"), (dict(label_smoothing=float("nan")), "label_smoothing"),
    (dict(focal_gamma=-1.0), "focal_gamma"), (dict(focal_gamma=float("nan")), "focal_gamma"), (dict(focal_gamma=float("inf")), "focal_gamma"),
    (dict(kind=2), "kind"), (dict(kind=-1), "kind"), (dict(reduction=2), "reduction"), (dict(reduction=-1), "reduction"),
    (dict(kind=nat.LOSS_FOCAL, focal_gamma=2.0, label_smoothing=0.125), "label_smoothing"),
])
def test_the_entry_refuses_bad_options_before_any_hip_call(kw, word):
    assert _ex(_opts(**kw)) == nat.WW_EINVAL and word in _err()


def test_the_entry_refuses_bad_pointers_and_the_device_check_comes_last():
    o = _opts()
    for n in (0, -1, 2 ** 30 + 1):
        assert _ex(o, n=n) == nat.WW_EINVAL and "n " in _err()
    assert _ex(o, logits=None) == nat.WW_EINVAL and "null" in _err()
    assert _ex(o, labels=None) == nat.WW_EINVAL and "null" in _err()
    assert _ex(None) == nat.WW_EINVAL and "opts_host" in _err()
    assert _ex(o, logits=18) == nat.WW_EINVAL and "aligned" in _err()
    assert _ex(o, dlogits=18) == nat.WW_EINVAL and "aligned" in _err()
    assert _ex(o, loss=18) == nat.WW_EINVAL and "aligned" in _err()
    assert _ex(o, labels=20) == nat.WW_EINVAL and "aligned" in _err()
    assert _ex(o, stats=20) == nat.WW_EINVAL and "stats_dev" in _err()
    if not torch.cuda.is_available():
        for good in (o, _opts(kind=nat.LOSS_FOCAL, focal_gamma=2.0), _opts(w=(0.0, 0.0), label_smoothing=1.0, reduction=nat.REDUCE_SUM, ignore_index=1)):
            assert _ex(good, logits=20, dlogits=36, loss=4) == nat.WW_ENODEVICE                # 4-byte alignment is enough


# ---- ops ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(weight=(1.0,)), dict(weight=(1.0, 2.0, 3.0)), dict(weight=(1.0, -1.0)), dict(weight=(float("nan"), 1.0)), dict(weight=(float("inf"), 1.0)),
    dict(weight=torch.ones(3)), dict(weight=torch.ones(2, 1)), dict(weight=5.0), dict(label_smoothing=-0.1), dict(label_smoothing=1.5),
    dict(label_smoothing=float("nan")), dict(label_smoothing="0.1"), dict(ignore_index=1.5), dict(ignore_index=None), dict(reduction="max"),
    dict(reduction=None), dict(focal_gamma=-0.5), dict(focal_gamma=float("inf")), dict(focal_gamma=float("nan")), dict(focal_gamma="2"),
    dict(focal_gamma=2.0, label_smoothing=0.125),
])
def test_ops_refuse_bad_options_before_looking_at_a_tensor(kw):
    z, y = torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64)                    # CPU tensors: a device check would raise RuntimeError
    with pytest.raises(ValueError):
        ops.ce_loss(z, y, **kw)
    with pytest.raises(ValueError):
        ops.loss_opts(**kw)


def test_reduction_none_is_not_implemented_and_defaults_are_the_plain_call():
    with pytest.raises(NotImplementedError):
        ops.ce_loss(torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64), reduction="none")
    assert ops.loss_opts() is None
    assert ops.loss_opts(weight=None, label_smoothing=0.0, ignore_index=-100, reduction="mean", focal_gamma=None) is None
    o = ops.loss_opts(weight=torch.tensor([0.25, 4.0]), label_smoothing=0.125, ignore_index=1, reduction="sum")
    assert (tuple(o.class_weight), o.label_smoothing, o.focal_gamma, o.ignore_index, o.kind, o.reduction) == ((0.25, 4.0), 0.125, 0.0, 1, 0, 1)
    o = ops.loss_opts(focal_gamma=2)
    assert (tuple(o.class_weight), o.label_smoothing, o.focal_gamma, o.ignore_index, o.kind, o.reduction) == ((1.0, 1.0), 0.0, 2.0, -100, 1, 0)
    for kw in (dict(weight=(1.0, 1.0)), dict(ignore_index=-1), dict(reduction="sum"), dict(label_smoothing=0.125), dict(focal_gamma=0.0)):
        assert ops.loss_opts(**kw) is not None                                     # any option given: the extended entry


# ---- FocalLoss -------------------------------------------------------------------------------------------------------------------------
def test_focal_loss_refuses_bad_arguments():
    for kw in (dict(gamma=-1.0), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(gamma="2"), dict(weight=(1.0,)), dict(weight=(1.0, -2.0)),
               dict(weight=torch.ones(3)), dict(reduction="max"), dict(ignore_index=0.5)):
        with pytest.raises(ValueError):
            pkg.FocalLoss(**kw)
    crit = pkg.FocalLoss()
    assert (crit.gamma, crit.weight, crit.reduction, crit.ignore_index) == (2.0, None, "mean", -100)
    with pytest.raises(ValueError):
        crit(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        crit(torch.zeros(4, 2), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        crit(torch.zeros(4, 2), torch.zeros(4))
    assert pkg.FocalLoss is pkg.loss.FocalLoss and pkg.balanced_class_weights is pkg.loss.balanced_class_weights
    assert "weight" in dict(pkg.FocalLoss(weight=(0.25, 4.0)).named_buffers())


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
@pytest.mark.parametrize("weight", [None, (0.25, 4.0)])
@pytest.mark.parametrize("gamma", ref.GAMMAS)
def test_focal_loss_forward_against_float64_autograd(gamma, weight, reduction):
    z, y = ref.case_inputs(257, "mixed")
    zt = torch.from_numpy(z).double().requires_grad_()
    crit = pkg.FocalLoss(gamma, weight=None if weight is None else torch.tensor(weight, dtype=torch.float64), reduction=reduction)
    out = crit(zt, torch.from_numpy(y))
    out.sum().backward()
    want = ref.loss(z, y, weight or (1.0, 1.0), reduction="sum" if reduction == "none" else reduction, focal_gamma=gamma)
    assert float(out.detach().sum()) == pytest.approx(want["loss"], rel=1e-13)
    g = zt.grad.numpy()
    assert np.isfinite(g).all()                                                    # also at +-160, where q underflows in float32
    assert np.abs(g - want["dlogits"]).max() * want["denom"] <= 1e-12 * max(1.0, gamma) * 320.0
    if reduction == "none":
        assert out.shape == (257,) and torch.all(out[torch.from_numpy(y) == -100] == 0.0)
    # targets of [n, 1] are squeezed as the reference's are; float32 stays finite at the extremes as well
    z32 = torch.from_numpy(z).requires_grad_()
    pkg.FocalLoss(gamma, reduction=reduction)(z32, torch.from_numpy(y)[:, None]).sum().backward()
    assert torch.isfinite(z32.grad).all()


def test_focal_loss_with_gamma_0_is_cross_entropy():
    z, y = ref.case_inputs(65, "mixed")
    zt, yt = torch.from_numpy(z).double(), torch.from_numpy(y)
    w = torch.tensor([0.25, 4.0], dtype=torch.float64)
    assert float(pkg.FocalLoss(0.0)(zt, yt)) == pytest.approx(float(nn.functional.cross_entropy(zt, yt)), rel=1e-13)
    assert float(pkg.FocalLoss(0.0, weight=w, reduction="sum")(zt, yt)) == pytest.approx(float(nn.functional.cross_entropy(zt, yt, weight=w, reduction="sum")), rel=1e-13)


# ---- the restatement against torch on the CPU -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.SIZES)
def test_restatement_agrees_with_torch_within_the_caps(n):
    for case in ref.kernel_cases(n):
        z, y = ref.case_inputs(n, case["labels"], case["extra"])
        want = ref.restate(case, z, y)
        lt, dt = ref.torch_reference(case, z, y, torch.device("cpu"), pkg.FocalLoss)
        if not want["denom"] > 0.0:
            assert lt != lt and want["loss"] != want["loss"] and not want["dlogits"].any(), case["tag"]     # NaN on both sides
            continue
        focal = "focal_gamma" in case["opts"]
        assert ref.loss_error(lt, want["loss"]) <= (ref.CAP_FOCAL_LOSS if focal else ref.CAP_CE_LOSS), case["tag"]
        assert ref.dlogits_error(dt, want) <= (ref.CAP_FOCAL_DLOGITS if focal else ref.CAP_CE_DLOGITS), case["tag"]


def test_restatement_with_unit_options_is_trainer_refs_cross_entropy():
    import trainer_ref
    z, y = trainer_ref.ce_inputs(257, seed=1)
    l64, d64, c64 = trainer_ref.ce(z, y)
    got = ref.loss(z, y)
    assert got["loss"] == pytest.approx(l64, rel=1e-15) and np.abs(got["dlogits"] - d64).max() <= 1e-16 and got["correct"] == c64
    y2 = y.copy()
    y2[::3] = -100                                                                 # ignored: out of the denominator, not bad
    y2[1::3] = 7                                                                   # bad: out of the denominator too, and counted
    got = ref.loss(z, y2)
    keep = (y2 == 0) | (y2 == 1)
    assert got["loss"] == pytest.approx(trainer_ref.ce(z[keep], y[keep])[0], rel=1e-14)
    assert got["bad"] == int((y2 == 7).sum()) and got["counted"] == int(keep.sum()) and not got["dlogits"][~keep].any()
    got = ref.loss(z, y, ignore_index=1)                                           # tested first: class 1 itself may be ignored
    assert got["counted"] == int((y == 0).sum()) and got["bad"] == 0


# ---- balanced_class_weights --------------------------------------------------------------------------------------------------------------
def test_balanced_class_weights():
    y = [0] * 30 + [1] * 10
    w = pkg.balanced_class_weights(y)
    assert w.dtype == torch.float32 and w.tolist() == [float(np.float32(40 / 60)), 2.0]
    assert torch.equal(pkg.balanced_class_weights(torch.tensor(y)), w) and torch.equal(pkg.balanced_class_weights(np.array(y).reshape(-1, 1)), w)
    nn.CrossEntropyLoss(weight=w)(torch.zeros(40, 2), torch.tensor(y))
    for bad in ([0, 0, 0], [1, 1], [0, 1, 2], [], [0.0, 1.0]):
        with pytest.raises(ValueError):
            pkg.balanced_class_weights(bad)


# ---- class-balanced epochs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pos, n_neg, f", [(5, 100, 0.5), (5, 100, 0.25), (100, 5, 0.5), (3, 4, 0.5), (1, 1, 0.5), (7, 50, 0.001), (7, 50, 0.999),
                                             (40, 40, 0.3)])
def test_balanced_order_counts(n_pos, n_neg, f):
    rng = np.random.default_rng(n_pos)
    y = np.array([1] * n_pos + [0] * n_neg)
    rng.shuffle(y)
    n = len(y)
    k = min(max(int(f * n + 0.5), 1), n - 1)
    torch.manual_seed(5)
    idx = pkg.balanced_order(y, f)
    assert idx.dtype == torch.int64 and idx.shape == (n,)
    idx = idx.numpy()
    assert int((y[idx] == 1).sum()) == k and int((y[idx] == 0).sum()) == n - k
    for cls in (0, 1):                                                             # within a class no item leads another by more than one
        counts = np.bincount(idx[y[idx] == cls], minlength=n)[y == cls]
        assert counts.max() - counts.min() <= 1
    torch.manual_seed(5)
    assert np.array_equal(pkg.balanced_order(torch.from_numpy(y), f).numpy(), idx)      # a seeded call repeats
    assert not np.array_equal(pkg.balanced_order(y, f).numpy(), idx) or n <= 3            # and the next epoch is another draw


def test_balanced_order_draws_positives_then_negatives_then_the_mix():
    y = np.array([0, 1, 0, 0, 1, 0, 0, 0])
    torch.manual_seed(9)
    got = pkg.balanced_order(y, 0.5)
    torch.manual_seed(9)
    pos, neg = torch.tensor([1, 4]), torch.tensor([0, 2, 3, 5, 6, 7])
    p = torch.cat([pos[torch.randperm(2)], pos[torch.randperm(2)]])[:4]
    q = neg[torch.randperm(6)][:4]
    assert torch.equal(got, torch.cat([p, q])[torch.randperm(8)])


def test_balanced_order_refusals():
    for f in (0.0, 1.0, -0.5, 1.5, float("nan"), None, "0.5", True):
        with pytest.raises(ValueError):
            pkg.balanced_order([0, 1, 0], f)
    for labels in ([0, 0, 0], [1, 1], [0, 1, 2], [0, -100, 1], [0.0, 1.0], []):
        with pytest.raises(ValueError):
            pkg.balanced_order(labels, 0.5)


class _Dataset:
    def __init__(self, labels):
        self.labels = list(labels)

    def __len__(self):
        return len(self.labels)


class _Bank:
    """What BankLoader.order() reads of a ClipBank: three clip entries and a stream entry of four windows."""
    n_items = 7
    labels = np.array([1, 0, 0, 0], np.int64)

    @staticmethod
    def item_entries():
        return np.array([0, 1, 2, 3, 3, 3, 3], np.int64)


def test_loaders_order_without_positive_fraction_is_what_it_was():
    ds = _Dataset([1] * 5 + [0] * 32)
    for loader, n in ((GpuBatchLoader(ds, 16, shuffle=True), 37), (BankLoader(_Bank, 4, shuffle=True), 7),
                      (GpuBatchLoader(ds, 16, shuffle=True, positive_fraction=None), 37)):
        assert loader.positive_fraction is None
        torch.manual_seed(3)
        got = loader.order()
        torch.manual_seed(3)
        assert got == torch.randperm(n).tolist()                                   # the parent's one draw
    torch.manual_seed(3)
    got = GpuBatchLoader(ds, 16, shuffle=True, drop_last=True).order()
    torch.manual_seed(3)
    assert got == torch.randperm(37).tolist()[:32]
    assert GpuBatchLoader(ds, 16).order() == list(range(37)) and BankLoader(_Bank, 4).order() == list(range(7))


def test_loaders_with_positive_fraction():
    ds = _Dataset([1] * 5 + [0] * 32)
    loader = GpuBatchLoader(ds, 16, shuffle=True, positive_fraction=0.5, drop_last=True)
    torch.manual_seed(4)
    idx = loader.order()
    torch.manual_seed(4)
    assert idx == pkg.balanced_order(ds.labels, 0.5).tolist()[:32] and len(loader) == 2
    full = GpuBatchLoader(ds, 16, shuffle=True, positive_fraction=0.5).order()
    assert len(full) == 37 and sum(ds.labels[i] for i in full) == 19               # int(0.5 * 37 + 0.5)
    bl = BankLoader(_Bank, 4, shuffle=True, positive_fraction=0.5)
    torch.manual_seed(4)
    idx = bl.order()
    torch.manual_seed(4)
    assert idx == pkg.balanced_order(_Bank.labels[_Bank.item_entries()], 0.5).tolist()
    assert sum(1 for i in idx if i == 0) == 4                                      # the one positive item, four times in seven
    for make in (lambda **kw: GpuBatchLoader(ds, 16, **kw), lambda **kw: BankLoader(_Bank, 4, **kw)):
        with pytest.raises(ValueError, match="shuffle"):
            make(shuffle=False, positive_fraction=0.5)
        for f in (0.0, 1.0, 2, "half"):
            with pytest.raises(ValueError):
                make(shuffle=True, positive_fraction=f)
    with pytest.raises(ValueError, match="missing"):
        GpuBatchLoader(_Dataset([0] * 8), 4, shuffle=True, positive_fraction=0.5).order()
    with pytest.raises(NotImplementedError):
        pkg.DataLoader(torch.utils.data.TensorDataset(torch.zeros(4)), batch_size=2, shuffle=True, positive_fraction=0.5)
    assert len(pkg.DataLoader(torch.utils.data.TensorDataset(torch.zeros(4)), batch_size=2)) == 2
