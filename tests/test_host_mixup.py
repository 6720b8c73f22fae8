"""Mixup and the soft-target cross-entropy without a GPU: the two C entries are bound and refuse every bad
argument before any HIP call, naming the field; the float64 restatement of tests/mixup_ref.py against torch on the CPU; the draws of
AudioProcessor.mixup_plan; check_mixup_config; and the device refusals of the Python surface."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import loss_ref
import mixup_ref as ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import ops
from wakeword_jupyterlab_amd.config import MixupConfig, check_mixup_config

L = nat.lib
U = ref.U


def _err():
    return (L.ww_last_error() or b"").decode()


# ---- the C entries -------------------------------------------------------------------------------------------------------------------
def test_abi_stays_4_and_both_entries_are_bound():
    assert L.ww_abi_version() == 4 == nat.ABI_VERSION
    assert nat.PROTOTYPES["ww_ce_loss_soft_f32"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(nat.LossOpts)] + [C.c_void_p] * 4)
    assert nat.PROTOTYPES["ww_mixup_f32"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32] + [C.c_void_p] * 5)
    assert L.ww_ce_loss_soft_f32.argtypes == nat.PROTOTYPES["ww_ce_loss_soft_f32"][1]
    assert L.ww_mixup_f32.argtypes == nat.PROTOTYPES["ww_mixup_f32"][1]
    assert C.sizeof(nat.LossOpts) == 48 and C.sizeof(nat.LossStats) == 48           # the structs keep their sizes


def _opts(**kw):
    o = nat.LossOpts()
    o.class_weight[0], o.class_weight[1] = kw.pop("w", (0.25, 4.0))
    o.label_smoothing, o.focal_gamma, o.ignore_index, o.kind, o.reduction = 0.0, 0.0, -100, nat.LOSS_CE, nat.REDUCE_MEAN
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _soft(opts, logits=None, targets=None, n=4, dlogits=None, loss=None, stats=None):
    return L.ww_ce_loss_soft_f32(logits, targets, n, None if opts is None else C.byref(opts), dlogits, loss, stats, None)


@pytest.mark.parametrize("kw, word", [
    (dict(kind=nat.LOSS_FOCAL, focal_gamma=2.0), "kind"), (dict(kind=2), "kind"), (dict(ignore_index=1), "ignore_index"),
    (dict(ignore_index=-1), "ignore_index"), (dict(w=(-1.0, 1.0)), "class_weight[0]"), (dict(w=(1.0, float("nan"))), "class_weight[1]"),
    (dict(w=(float("inf"), 1.0)), "class_weight[0]"), (dict(label_smoothing=-0.1), "label_smoothing"), (dict(label_smoothing=1.5), "label_smoothing"),
    (dict(label_smoothing=float("nan")), "label_smoothing"), (dict(reduction=2), "reduction"), (dict(reduction=-1), "reduction"),
])
def test_the_soft_loss_refuses_bad_options_with_null_device_pointers(kw, word):
    """Every device pointer is NULL: the option is named all the same, so the check ran before any HIP call (and before the pointers')."""
    assert _soft(_opts(**kw)) == nat.WW_EINVAL and word in _err()


def test_the_soft_loss_refuses_bad_n_and_pointers_and_the_device_check_comes_last():
    for n in (0, -1, 2 ** 30 + 1):
        assert _soft(_opts(), n=n) == nat.WW_EINVAL and "n " in _err()
    assert _soft(_opts()) == nat.WW_EINVAL and "null" in _err()
    assert _soft(None) == nat.WW_EINVAL and "null" in _err()                          # NULL options are the defaults, not an error
    assert _soft(_opts(), logits=16) == nat.WW_EINVAL and "null" in _err()
    for kw in (dict(logits=18), dict(targets=18), dict(dlogits=18), dict(loss=18)):
        assert _soft(_opts(), **{"logits": 16, "targets": 32, **kw}) == nat.WW_EINVAL and "aligned" in _err()
    assert _soft(_opts(), logits=16, targets=32, stats=20) == nat.WW_EINVAL and "stats_dev" in _err()
    if not torch.cuda.is_available():
        for good in (None, _opts(), _opts(w=(0.0, 0.0), label_smoothing=1.0, reduction=nat.REDUCE_SUM)):
            assert _soft(good, logits=20, targets=36, dlogits=52, loss=4) == nat.WW_ENODEVICE    # 4-byte alignment is enough


def _mix(mel=4096, out=1 << 20, B=4, T=8, labels=64, partner=128, lam=256, targets=512):
    return L.ww_mixup_f32(mel, out, B, T, labels, partner, lam, targets, None)


def test_mixup_refuses_bad_arguments_before_any_hip_call():
    for B in (0, -1, 2 ** 30 + 1):
        assert _mix(None, None, B=B, labels=None, partner=None, lam=None, targets=None) == nat.WW_EINVAL and "B " in _err()
    for T in (0, -3, 64, 1000):
        assert _mix(None, None, T=T, labels=None, partner=None, lam=None, targets=None) == nat.WW_EINVAL and "T " in _err()
    for kw in (dict(mel=None), dict(out=None), dict(labels=None), dict(partner=None), dict(lam=None), dict(targets=None)):
        assert _mix(**kw) == nat.WW_EINVAL and "null" in _err()
    for kw in (dict(mel=4098), dict(out=(1 << 20) + 1), dict(partner=130), dict(lam=258), dict(targets=513), dict(labels=68)):
        assert _mix(**kw) == nat.WW_EINVAL and "aligned" in _err()
    row = 4 * 80 * 8 * 4                                                             # bytes of a batch of 4 rows at T = 8
    for mel, out in ((4096, 4096), (4096, 4096 + row - 4), (4096 + row - 4, 4096), (4096, 4096 + 4)):
        assert _mix(mel=mel, out=out) == nat.WW_EINVAL and "overlap" in _err()
    if not torch.cuda.is_available():
        assert _mix(mel=4096, out=4096 + row) == nat.WW_ENODEVICE                     # adjacent is not overlapping
        assert _mix(mel=4100, out=4100 + row, T=8) == nat.WW_ENODEVICE                # 4-byte alignment is enough
        assert _mix(T=63) == nat.WW_ENODEVICE and _mix(T=1) == nat.WW_ENODEVICE


# ---- the restatement against torch on the CPU ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", loss_ref.SIZES)
def test_soft_restatement_agrees_with_torch_float64(n):
    z, t = ref.soft_inputs(n)
    for case in ref.soft_cases(n):
        want = ref.restate(case, z, t)
        lt, dt = ref.torch_reference(case, z, t, torch.device("cpu"), torch.float64)
        assert abs(lt - want["loss"]) <= 1e-12 * max(1.0, abs(want["loss"])), case["tag"]
        assert np.abs(dt - want["dlogits"]).max() <= 1e-12, case["tag"]
        assert want["counted"] == n and want["bad"] == 0


@pytest.mark.parametrize("n", loss_ref.SIZES)
def test_torch_float32_on_the_cpu_stays_under_the_caps(n):
    z, t = ref.soft_inputs(n)
    for case in ref.soft_cases(n):
        want = ref.restate(case, z, t)
        lt, dt = ref.torch_reference(case, z, t, torch.device("cpu"))
        assert loss_ref.loss_error(lt, want["loss"]) <= ref.CAP_SOFT_LOSS, case["tag"]
        assert loss_ref.dlogits_error(dt, want) <= ref.CAP_SOFT_DLOGITS, case["tag"]


def test_soft_restatement_on_one_hot_rows_is_the_hard_loss_and_bad_rows_are_left_out():
    import trainer_ref
    z, y = trainer_ref.ce_inputs(257, seed=1)
    l64, d64, c64 = trainer_ref.ce(z, y)
    got = ref.soft_loss(z, ref.one_hot(y))
    assert got["loss"] == pytest.approx(l64, rel=1e-15) and np.abs(got["dlogits"] - d64).max() <= 1e-16 and got["correct"] == c64
    for w, eps, red in ((0.25, 4.0), 0.125, "mean"), ((0.25, 4.0), 0.0, "sum"):
        hard = loss_ref.loss(z, y, w, eps, reduction=red)
        soft = ref.soft_loss(z, ref.one_hot(y), w, eps, red)
        scale = hard["denom"] / soft["denom"]                                      # the weighted mean against the mean over rows
        assert soft["loss"] == pytest.approx(hard["loss"] * scale, rel=1e-13)
        assert np.abs(soft["dlogits"] - hard["dlogits"] * scale).max() <= 1e-14
    t = ref.one_hot(y)
    t[0], t[100], t[256] = (np.nan, 0.5), (np.inf, 0.0), (-0.25, 1.25)
    keep = np.ones(257, bool)
    keep[[0, 100, 256]] = False
    got = ref.soft_loss(z, t)
    assert got["bad"] == 3 and got["counted"] == 254 and not got["dlogits"][~keep].any()
    assert got["loss"] == pytest.approx(trainer_ref.ce(z[keep], y[keep])[0], rel=1e-14)
    none = ref.soft_loss(z, np.full((257, 2), np.nan, np.float32))
    assert none["loss"] != none["loss"] and not none["dlogits"].any() and ref.soft_loss(z, t * np.nan, reduction="sum")["loss"] == 0.0


def test_mixup_restatement_rules():
    mel, labels, partner, lam = ref.mix_inputs(5, 8)
    out, targets, mixed = ref.mixup(mel, labels, partner, lam)
    assert mixed[[0, 2, 3, 4]].all() and np.isnan(targets[0]).all()                 # row 0's partner is row 1
    assert np.isnan(targets[1]).all() and np.isnan(targets[2]).all()                # label 7 on the row, and on the partner of a mixed row
    assert targets[3].tolist() == [0.875, 0.125]                                    # labels 0 and 1
    assert targets[4].tolist() == [0.0, 1.0]                                        # mixed with itself: the same class, the exact one-hot
    assert np.array_equal(out[~mixed], mel[~mixed].astype(np.float64))
    bad = partner.copy()
    bad[3] = 5
    out2, t2, m2 = ref.mixup(mel, labels, bad, lam)
    assert not m2[3] and np.isnan(t2[3]).all() and np.array_equal(out2[3], mel[3].astype(np.float64))


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
class _Counting(random.Random):
    """python's generator with its draws counted by kind (betavariate draws through random() internally: counted once, as one draw)."""

    def __init__(self, seed):
        super().__init__(seed)
        self.calls = {"sample": 0, "random": 0, "betavariate": 0}
        self._inside = 0

    def sample(self, *a, **kw):
        self.calls["sample"] += 1
        self._inside += 1
        try:
            return super().sample(*a, **kw)
        finally:
            self._inside -= 1

    def betavariate(self, *a):
        self.calls["betavariate"] += 1
        self._inside += 1
        try:
            return super().betavariate(*a)
        finally:
            self._inside -= 1

    def getrandbits(self, k):                      # defined here so that sample() keeps drawing bits, as the plain generator does
        return super().getrandbits(k)

    def random(self):
        if not self._inside:
            self.calls["random"] += 1
        return super().random()


def _plan(monkeypatch, seed, B, cfg=MixupConfig, bad=None):
    gen = _Counting(seed)
    for name in ("sample", "random", "betavariate"):
        monkeypatch.setattr(random, name, getattr(gen, name))
    p = pkg.AudioProcessor()
    p.set_mixup(cfg)
    partner, lam = p.mixup_plan(B, bad=bad)
    return partner, lam, gen.calls


@pytest.mark.parametrize("B", [1, 2, 16, 257])
def test_mixup_plan_repeats_and_draws_one_sample_B_coins_and_one_beta_per_chosen_row(B, monkeypatch):
    partner, lam, calls = _plan(monkeypatch, 11, B)
    partner2, lam2, _ = _plan(monkeypatch, 11, B)
    assert np.array_equal(partner, partner2) and np.array_equal(lam, lam2)           # seeded, it repeats
    assert partner.dtype == np.int32 and lam.dtype == np.float32 and partner.shape == lam.shape == (B,)
    assert calls["sample"] == 1 and calls["random"] == B and calls["betavariate"] >= int((lam != 1.0).sum())
    # the same draws by hand, in the documented order
    gen = random.Random(11)
    want_p = gen.sample(range(B), B)
    want = np.ones(B, np.float32)
    chosen = 0
    for i in range(B):
        if gen.random() < MixupConfig.PROB:
            chosen += 1
            v = np.float32(gen.betavariate(MixupConfig.ALPHA, MixupConfig.ALPHA))
            want[i] = np.float32(1.0) - v if v < np.float32(0.5) else v
    assert calls["betavariate"] == chosen and np.array_equal(lam, want)
    assert (lam >= 0.5).all() and (lam <= 1.0).all()                                 # DOMINANT
    mixed = lam != 1.0
    assert np.array_equal(partner[mixed], np.asarray(want_p, np.int32)[mixed]) and np.array_equal(partner[~mixed], np.arange(B)[~mixed])


def test_mixup_plan_options_and_bad_rows(monkeypatch):
    class Always(MixupConfig):
        PROB = 1.0

    class Never(MixupConfig):
        PROB = 0.0

    class Either(MixupConfig):
        PROB = 1.0
        DOMINANT = False

    B = 64
    partner, lam, calls = _plan(monkeypatch, 5, B, Never)
    assert calls == {"sample": 1, "random": B, "betavariate": 0}                     # the identity plan still draws its sample and coins
    assert np.array_equal(partner, np.arange(B)) and (lam == 1.0).all()
    partner, lam, calls = _plan(monkeypatch, 5, B, Always)
    assert calls["betavariate"] == B and (lam >= 0.5).all()
    _, lam_e, _ = _plan(monkeypatch, 5, B, Either)
    assert (lam_e < 0.5).any() and np.array_equal(np.where(lam_e < np.float32(0.5), np.float32(1.0) - lam_e, lam_e), lam)
    bad = np.zeros(B, bool)
    bad[[3, 17]] = True
    partner_b, lam_b, calls_b = _plan(monkeypatch, 5, B, Always, bad=bad)
    assert calls_b == calls                                                          # the fix-up draws nothing
    hit = bad | bad[partner]                                                         # bad rows, and rows whose drawn partner is bad
    assert (lam_b[hit] == 1.0).all() and np.array_equal(partner_b[hit], np.arange(B)[hit])
    assert np.array_equal(lam_b[~hit], lam[~hit]) and np.array_equal(partner_b[~hit], partner[~hit])
    with pytest.raises(ValueError):
        pkg.AudioProcessor().mixup_plan(0)
    with pytest.raises(ValueError):
        pkg.AudioProcessor().mixup_plan(4, bad=np.zeros(3, bool))


# ---- config and the Python surface ----------------------------------------------------------------------------------------------------------
def test_check_mixup_config_refusals_and_the_switch():
    assert (MixupConfig.PROB, MixupConfig.ALPHA, MixupConfig.DOMINANT) == (0.5, 0.2, True) and pkg.MixupConfig is MixupConfig
    check_mixup_config(MixupConfig)
    for field, value in (("PROB", -0.1), ("PROB", 1.5), ("PROB", float("nan")), ("PROB", "0.5"), ("ALPHA", 0.0), ("ALPHA", -1.0),
                         ("ALPHA", float("inf")), ("ALPHA", float("nan")), ("ALPHA", None), ("ALPHA", True)):
        bad = type("Bad", (MixupConfig,), {field: value})
        with pytest.raises(ValueError):
            check_mixup_config(bad)
        with pytest.raises(ValueError):
            pkg.AudioProcessor().set_mixup(bad)
    p = pkg.AudioProcessor()
    assert p.mixup is None
    assert p.set_mixup(MixupConfig) is MixupConfig and p.mixup is MixupConfig
    assert p.set_mixup(None) is None and p.mixup is None


def test_python_wrappers_refuse_cpu_tensors_and_bad_options():
    z, t = torch.zeros(4, 2), torch.full((4, 2), 0.5)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        ops.soft_ce_loss(z, t)
    mel = torch.zeros(4, 1, 80, 8)
    y, partner, lam = torch.zeros(4, dtype=torch.int64), torch.arange(4, dtype=torch.int32), torch.ones(4)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        ops.mixup(mel, y, partner, lam)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        ops.mixup_into(mel, y, partner, lam, torch.zeros_like(mel), torch.zeros(4, 2))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        pkg.AudioProcessor().mixup_batch(mel, y)
    # options are checked before a tensor is looked at
    with pytest.raises(NotImplementedError):
        ops.soft_ce_loss(z, t, focal_gamma=2.0)
    with pytest.raises(NotImplementedError):
        ops.soft_ce_loss(z, t, reduction="none")
    for kw in (dict(weight=(1.0,)), dict(weight=(1.0, -1.0)), dict(label_smoothing=1.5), dict(reduction="max")):
        with pytest.raises(ValueError):
            ops.soft_ce_loss(z, t, **kw)
    with pytest.raises(ValueError):
        ops.soft_loss_opts(ignore_index=1)
    assert ops.soft_loss_opts() is None and ops.soft_loss_opts(reduction="sum").reduction == nat.REDUCE_SUM
    # ops.ce_loss still refuses float targets: class probabilities have an entry of their own
    with pytest.raises((TypeError, RuntimeError)):
        ops.ce_loss(z, t)


# ---- the loaders' host logic: what is drawn, what is called, in which order --------------------------------------------------------------
class _Proc(pkg.AudioProcessor):
    """The processor's device work replaced by host stand-ins, as in tests/test_host_specaug.py."""

    def augment_batch(self, pcm, plans=None, config=None):
        self.log.append(("augment", random.getrandbits(32)))
        return pcm

    def mel_batch(self, pcm, normalize=True):
        self.log.append(("mel",))
        return torch.arange(pcm.shape[0] * 80 * 8, dtype=torch.float32).reshape(pcm.shape[0], 1, 80, 8) * -0.01


class _Bank:
    """What BankLoader reads of a ClipBank: seven entries, one of them a placeholder for an unreadable file."""
    n_items = 7
    kinds = np.zeros(7, np.int64)
    ok = np.array([True] * 5 + [False, True])
    labels = np.arange(7, dtype=np.int64) % 2

    def __init__(self, proc):
        self.processor = proc

    def item_entries(self):
        return np.arange(7, dtype=np.int64)

    def draw_starts(self, entries):
        return np.array([random.randint(0, 9) for _ in entries], dtype=np.int64)

    def _gather(self, entries, starts, norms):
        return torch.zeros(len(entries), 4000)


def _epoch(proc, augment, monkeypatch):
    from wakeword_jupyterlab_amd import bank as bankmod
    proc.log = []
    calls = []

    def fake(mel, labels, partner, lam, out=None):
        calls.append((mel.clone(), labels.clone(), partner.clone(), lam.clone()))
        out64, targets, _ = ref.mixup(mel.numpy(), labels.numpy(), partner.numpy(), lam.numpy())
        return torch.from_numpy(out64.astype(np.float32)), torch.from_numpy(targets)
    monkeypatch.setattr(ops, "mixup", fake)
    random.seed(11)
    loader = bankmod.BankLoader(_Bank(proc), 3, augment=augment)
    batches = [(d.clone(), t.clone(), loader.last_entries.copy(), loader.last_labels.clone()) for d, t in loader]
    return batches, calls, random.getstate(), list(proc.log)


def test_bank_loader_host_logic_mixes_last_and_is_untouched_when_mixup_is_off(monkeypatch):
    class Always(MixupConfig):
        PROB = 1.0

    proc = _Proc()
    control = {aug: _epoch(proc, aug, monkeypatch) for aug in (False, True)}       # no config: the loader as it was
    assert all(c[1] == [] for c in control.values())
    assert all(t.dtype == torch.int64 and t.shape[1] == 1 and torch.equal(y, t[:, 0]) for _, t, _, y in control[True][0])
    proc.set_mixup(Always)
    off = _epoch(proc, False, monkeypatch)                                         # augment=False: nothing drawn, nothing called
    assert off[1] == [] and off[2] == control[False][2] and off[3] == control[False][3]
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(off[0], control[False][0]))
    on = _epoch(proc, True, monkeypatch)
    assert len(on[1]) == 3 and [x[0] for x in on[3]] == [x[0] for x in control[True][3]]     # one call per batch, after the same calls
    # the replay: starts, augment_batch's draw, then the plan of the batch
    random.seed(11)
    plain = pkg.AudioProcessor()
    plain.set_mixup(Always)
    for k, nb in enumerate((3, 3, 1)):
        for _ in range(nb):
            random.randint(0, 9)
        random.getrandbits(32)
        bad = ~_Bank.ok[3 * k:3 * k + nb]
        partner, lam = plain.mixup_plan(nb, bad=bad)
        mel, labels, got_partner, got_lam = on[1][k]
        assert np.array_equal(got_partner.numpy(), partner) and np.array_equal(got_lam.numpy(), lam)
        assert got_partner.dtype == torch.int32 and got_lam.dtype == torch.float32 and labels.dtype == torch.int64
        assert torch.equal(mel, control[True][0][k][0])                            # mixup sees the batch after bad rows were zeroed
        data, target, entries, own = on[0][k]
        assert target.dtype == torch.float32 and target.shape == (nb, 2) and torch.equal(own, labels)
        assert np.array_equal(own.numpy(), _Bank.labels[3 * k:3 * k + nb])
        want_entries = np.where(bad | (lam != 1.0), -1, np.arange(3 * k, 3 * k + nb))
        assert np.array_equal(entries, want_entries) and entries.dtype == np.int64
    assert random.getstate() == on[2]
    assert not on[1][1][0][2].any() and on[1][1][3][2] == 1.0 and on[0][1][2][2] == -1       # entry 5: zeroed, unmixed, skipped by the ledger
    proc.set_mixup(None)
    again = _epoch(proc, True, monkeypatch)
    assert again[1] == [] and again[2] == control[True][2]
