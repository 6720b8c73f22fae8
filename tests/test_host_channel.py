"""Microphone-channel augmentation, everything that needs no GPU: the config validator, the record packing,
the C entry points' refusals before any HIP call, the Meta kernel, the processor's switch, the draws of python `random` with the switch
off and on, and the numpy restatement (tests/channel_ref.py) checked against itself."""
import random

import numpy as np
import pytest
import torch

import channel_ref as ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import bank as bankmod
from wakeword_jupyterlab_amd import ops
from wakeword_jupyterlab_amd.config import AugmentationConfig, ChannelConfig, SpecAugmentConfig, check_channel_config

SEEDS = (0, 1, 2 ** 63 + 12345, 2 ** 64 - 1)


def _cfg(**kw):
    return type("Cfg", (ChannelConfig,), kw)


def test_defaults_and_validator():
    c = ChannelConfig
    assert pkg.ChannelConfig is c
    assert ref.config_of(c) == ref.DEFAULTS
    check_channel_config(c)
    for ok in (_cfg(PROB=0), _cfg(PROB=1.0), _cfg(PEAKS=0), _cfg(PEAKS=4), _cfg(LOWPASS_HZ=(7600.0, 7600.0)), _cfg(DRIVE=(0.0, 8.0)),
               _cfg(SHELF_DB=0), _cfg(PEAK_Q=(4, 4)), _cfg(HIGHPASS_HZ=[20, 30])):
        check_channel_config(ok)
    for bad in (_cfg(PROB=-0.1), _cfg(PROB=1.5), _cfg(PROB=float("nan")), _cfg(DRIVE_PROB=2), _cfg(HIGHPASS_PROB=-1), _cfg(PEAK_PROB=True),
                _cfg(HIGHPASS_HZ=(0.0, 400.0)), _cfg(LOWPASS_HZ=(3000.0, 7601.0)), _cfg(PEAK_HZ=(-5.0, 100.0)), _cfg(LOW_SHELF_HZ=(400.0, 100.0)),
                _cfg(HIGH_SHELF_HZ=2000.0), _cfg(PEAK_Q=(0.0, 2.0)), _cfg(PEAK_Q=(-1.0, 2.0)), _cfg(PEAK_Q=(2.0, 0.5)), _cfg(PEAKS=5),
                _cfg(PEAKS=-1), _cfg(PEAKS=1.5), _cfg(DRIVE=(-0.5, 3.0)), _cfg(DRIVE=(0.5, 8.5)), _cfg(DRIVE=(3.0, 0.5)), _cfg(SHELF_DB=-1),
                _cfg(PEAK_DB=float("inf")), _cfg(PEAK_HZ=(100.0, float("nan"))), _cfg(HIGHPASS_HZ=(1e-50, 400.0)), _cfg(PEAK_Q=(0.5, 2e6)),
                _cfg(PEAK_Q=(1e-50, 2.0)), _cfg(DRIVE=(0.5, 1e50))):
        with pytest.raises(ValueError):
            check_channel_config(bad)
        with pytest.raises(ValueError):
            pkg.AudioProcessor().set_channel_effects(bad)


def test_pack_channel_plans_layout_identity_sections_and_refusals():
    full = {"highpass": 20.0, "low_shelf": (200.0, 4.0), "peaks": [(100.0, 6.0, 4.0), (900.0, -3.0, 1.0), (2500.0, 5.0, 0.7), (5000.0, -6.0, 2.0)],
            "high_shelf": (3000.0, -5.0), "lowpass": 3400.0, "drive": 2.5}
    rec = ops.pack_channel_plans([{}, {"peaks": [(1000.0, 6.0, 1.0)]}, full, {"drive": 1.0}, {"lowpass": 7600}])
    assert rec.dtype == np.float32 and rec.shape == (5, 48) and rec.flags["C_CONTIGUOUS"]
    assert rec.itemsize * rec.shape[1] == nat.lib.ww_channel_record_bytes() == 192
    ident = ref.is_identity(rec)
    assert ident[0].all() and ref.is_off(rec).tolist() == [True, False, False, False, False]
    assert rec[0].tolist() == [1, 0, 0, 0, 0] * 8 + [0] * 8
    assert ident[1].tolist() == [True, True, False] + [True] * 5 and not ident[2].any() and ident[3].all() and rec[3, 40] == 1.0
    assert (rec[:, 41:] == 0).all() and rec[2, 40] == 2.5
    # the coefficients are the restatement's float64 ones, rounded once
    want = np.concatenate([ref.coefficients("highpass", 20.0), ref.coefficients("low_shelf", 200.0, 4.0)] +
                          [ref.coefficients("peak", *p) for p in full["peaks"]] +
                          [ref.coefficients("high_shelf", 3000.0, -5.0), ref.coefficients("lowpass", 3400.0)])
    assert np.array_equal(rec[2, :40], want.astype(np.float32))
    for kind, args in (("highpass", (20.0,)), ("lowpass", (7500.0,)), ("peak", (100.0, -6.0, 4.0)), ("low_shelf", (100.0, 6.0)),
                       ("high_shelf", (5000.0, -6.0))):
        assert np.array_equal(ops.channel_coefficients(kind, *args), ref.coefficients(kind, *args))
        assert ref.pole_radius(ops.channel_coefficients(kind, *args)) < 1.0                  # stable
    # a few values that the cookbook forms must give: unit gain at DC for the shelves' far side, a peak's gain at its centre
    assert abs(ref.response(ref.coefficients("peak", 1000.0, 6.0, 1.0), 1000.0) - 10 ** (6 / 20)) < 1e-12
    assert abs(ref.response(ref.coefficients("low_shelf", 200.0, 6.0), 1e-6) - 10 ** (6 / 20)) < 1e-6
    assert abs(ref.response(ref.coefficients("high_shelf", 3000.0, -6.0), 8000.0) - 10 ** (-6 / 20)) < 1e-12
    assert abs(ref.response(ref.coefficients("highpass", 300.0), 300.0) - 2 ** -0.5) < 1e-12
    assert abs(ref.response(ref.coefficients("lowpass", 3400.0), 3400.0) - 2 ** -0.5) < 1e-12
    for bad in ([{"peaks": [(100.0, 1.0, 1.0)] * 5}], [{"highpass": 0.0}], [{"lowpass": 7601.0}], [{"peaks": [(100.0, 1.0, 0.0)]}],
                [{"drive": -1.0}], [{"drive": 8.5}], [{"treble": 3.0}], [{"high_shelf": (9000.0, 1.0)}]):
        with pytest.raises(ValueError):
            ops.pack_channel_plans(bad)
    assert ops.pack_channel_plans([]).shape == (0, 48)


def _struct(**kw):
    g = ops._channel_struct(ChannelConfig)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_entry_points_refuse_bad_arguments_before_touching_a_device():
    import ctypes as C
    L = nat.lib
    N = 4003
    buf = np.zeros(3 * N + 64, np.float32)
    a = (buf.ctypes.data + 15) // 16 * 16                                   # a 16-byte aligned host address: never dereferenced
    rec = a
    good = _struct()

    def apply(pcm_in=a, pcm_out=a, n=2, n_samples=N, stride=None, records=rec, cfg=good):
        return L.ww_channel_f32(pcm_in, pcm_out, n, n_samples, n_samples if stride is None else stride, records, 1,
                                None if cfg is None else C.byref(cfg), None)

    def draw(n=2, records=rec, cfg=good):
        return L.ww_channel_draw(1, n, None if cfg is None else C.byref(cfg), records, None)

    for bad_n in (3999, 16384, 32000, 0, -5):
        assert apply(n_samples=bad_n) == nat.WW_EUNSUPPORTED, bad_n
        assert b"n_samples" in L.ww_last_error()
    bad_cfgs = [_struct(prob=-0.01), _struct(prob=1.01), _struct(prob=float("nan")), _struct(highpass_prob=2.0), _struct(low_shelf_prob=-1.0),
                _struct(high_shelf_prob=1.5), _struct(peak_prob=-0.5), _struct(lowpass_prob=9.0), _struct(drive_prob=float("inf")),
                _struct(highpass_lo=0.0), _struct(lowpass_hi=7601.0), _struct(peak_lo=7000.0), _struct(peak_q_lo=0.0), _struct(peak_q_hi=0.1),
                _struct(peaks=5), _struct(peaks=-1), _struct(drive_lo=-0.5), _struct(drive_hi=8.5), _struct(drive_lo=4.0), _struct(shelf_db=-1.0),
                _struct(peak_db=float("nan"))]
    for call in (apply, draw):
        assert call(n=-1) == nat.WW_EINVAL
        for g in bad_cfgs:
            assert call(cfg=g) == nat.WW_EINVAL
        assert call(n=0, records=None) == nat.WW_OK                         # nothing to do: no launch, no device needed
    assert apply(records=None, cfg=None) == nat.WW_EINVAL and draw(cfg=None) == nat.WW_EINVAL      # a draw without a config
    assert apply(n=0, pcm_in=None, pcm_out=None) == nat.WW_OK
    assert apply(pcm_in=None) == nat.WW_EINVAL and apply(pcm_out=None) == nat.WW_EINVAL and draw(records=None) == nat.WW_EINVAL
    assert apply(pcm_in=a + 2) == nat.WW_EINVAL and apply(pcm_out=a + 1) == nat.WW_EINVAL
    assert apply(records=rec + 4) == nat.WW_EINVAL and draw(records=rec + 8) == nat.WW_EINVAL
    assert apply(stride=N - 1) == nat.WW_EINVAL
    nbytes = 2 * N * 4
    for shift in (4, nbytes - 4):                                           # partial overlap, from either side
        assert apply(pcm_out=a + shift) == nat.WW_EINVAL and b"overlap" in L.ww_last_error()
        assert apply(pcm_in=a + shift, pcm_out=a) == nat.WW_EINVAL
    if not torch.cuda.is_available():                                       # everything in order: only the device is missing
        assert apply() == nat.WW_ENODEVICE                                  # in place
        assert apply(pcm_out=a + nbytes) == nat.WW_ENODEVICE                # disjoint
        assert apply(cfg=None) == nat.WW_ENODEVICE                          # records given: no config needed
        assert apply(records=None) == nat.WW_ENODEVICE and draw() == nat.WW_ENODEVICE
        assert apply(n_samples=16000) == nat.WW_ENODEVICE and apply(n_samples=4000) == nat.WW_ENODEVICE
        assert apply(n_samples=16383) == nat.WW_ENODEVICE


def test_operator_schema_meta_kernel_and_cpu_refusal():
    ns = torch.ops.wakeword_amd
    assert str(ns.channel_effects.default._schema) == "wakeword_amd::channel_effects(Tensor pcm, Tensor records) -> Tensor"
    for shape in ((3, 16000), (5, 4000), (0, 16383), (2, 4003)):
        y = ns.channel_effects(torch.empty(shape, device="meta"), torch.empty((shape[0], 48), device="meta"))
        assert y.shape == shape and y.dtype == torch.float32 and y.device.type == "meta"
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)                 # noqa: E731
    for bad in (lambda: ns.channel_effects(m(3, 16384), m(3, 48)), lambda: ns.channel_effects(m(3, 3999), m(3, 48)),
                lambda: ns.channel_effects(m(3, 1, 16000), m(3, 48)), lambda: ns.channel_effects(m(3, 16000), m(2, 48)),
                lambda: ns.channel_effects(m(3, 16000), m(3, 47)), lambda: ns.channel_effects(m(3, 16000), m(3, 48, dtype=torch.float64)),
                lambda: ns.channel_effects(m(3, 16000, dtype=torch.float64), m(3, 48))):
        with pytest.raises(RuntimeError):
            bad()
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        ns.channel_effects(torch.zeros(2, 16000), torch.zeros(2, 48))


def test_python_wrappers_check_their_arguments():
    rec = torch.zeros(2, 48)
    with pytest.raises(RuntimeError):
        ops.channel_effects(torch.zeros(2, 16000), rec)                     # a CPU tensor
    with pytest.raises(RuntimeError):
        ops.channel_records(1, 4, device="cpu")
    with pytest.raises(ValueError):
        ops.channel_records(1, 4, _cfg(PEAKS=9), device="cuda")
    with pytest.raises(ValueError):
        ops.channel_records(1, -1, device="cuda")
    with pytest.raises(TypeError):
        ops.channel_effects(np.zeros((2, 16000), np.float32), rec)


def test_switch_is_off_by_default_and_mirrors_the_other_switches():
    p = pkg.AudioProcessor()
    assert p.channel_effects is None
    assert p.set_channel_effects(ChannelConfig) is ChannelConfig and p.channel_effects is ChannelConfig
    assert p.set_channel_effects(None) is None and p.channel_effects is None


class _Proc(pkg.AudioProcessor):
    """The processor's device work replaced by host stand-ins: the loaders' own logic (what is drawn, what is called, in which order) runs."""

    def augment_batch(self, pcm, plans=None, config=AugmentationConfig):
        self.log.append(("augment", random.getrandbits(32)))
        return pcm

    def mel_batch(self, pcm, normalize=True):
        self.log.append(("mel", float(pcm.sum())))
        return torch.ones(pcm.shape[0], 1, 80, 32)

    def load_clips_gpu(self, paths, normalize=True, lo=0, hi=None):
        self.log.append(("load", random.randint(0, 99)))                   # the crop start
        return torch.zeros(len(paths), 16000), np.ones(len(paths), bool)


class _Bank:
    """What BankLoader reads of a ClipBank: seven one-second entries, one of them a placeholder for an unreadable file."""
    n_items = 7
    kinds = np.zeros(7, np.int64)
    ok = np.array([True] * 6 + [False])
    labels = np.arange(7, dtype=np.int64) % 2

    def __init__(self, proc):
        self.processor = proc

    def item_entries(self):
        return np.arange(7, dtype=np.int64)

    def draw_starts(self, entries):
        return np.array([random.randint(0, 9) for _ in entries], dtype=np.int64)

    def _gather(self, entries, starts, norms):
        return torch.zeros(len(entries), 16000)


def _patch(monkeypatch):
    calls = []

    def chan(pcm, records=None, *, seed=None, config=None, out=None):
        calls.append(("channel", seed, config, out is pcm))
        pcm.fill_(2.0)
        return pcm

    def spec(mel, records=None, *, seed=None, config=None, out=None):
        calls.append(("spec", seed, config, out is mel))
        mel.fill_(5.0)
        return mel
    monkeypatch.setattr(ops, "channel_effects", chan)
    monkeypatch.setattr(ops, "spec_augment", spec)
    return calls


def _epoch(proc, augment, monkeypatch):
    proc.log = []
    calls = _patch(monkeypatch)
    random.seed(11)
    batches = [d.clone() for d, _ in bankmod.BankLoader(_Bank(proc), 3, augment=augment)]
    return batches, calls, random.getstate(), list(proc.log)


def test_bank_loader_host_logic_draws_one_seed_per_augmented_batch_and_nothing_otherwise(monkeypatch):
    proc = _Proc()
    control = {aug: _epoch(proc, aug, monkeypatch) for aug in (False, True)}       # no config: the loader as it was
    assert all(c[1] == [] for c in control.values())
    proc.set_channel_effects(ChannelConfig)
    off = _epoch(proc, False, monkeypatch)                                         # a validation loader: nothing drawn, nothing launched
    assert off[1] == [] and off[2] == control[False][2] and off[3] == control[False][3]
    assert all(torch.equal(x, y) for x, y in zip(off[0], control[False][0]))
    proc.set_spec_augment(SpecAugmentConfig)
    on = _epoch(proc, True, monkeypatch)
    assert [c[0] for c in on[1]] == ["channel", "spec"] * 3
    assert all(c[2] is (ChannelConfig if c[0] == "channel" else SpecAugmentConfig) and c[3] for c in on[1])
    assert [x[0] for x in on[3]] == [x[0] for x in control[True][3]]              # the same processor calls in the same order
    assert all(x[1] == 2.0 * 16000 * nb for x, nb in zip([x for x in on[3] if x[0] == "mel"], (3, 3, 1)))   # K1 saw the filtered rows
    # the replay: starts, augment_batch's draw, the channel seed, then SpecAugment's seed
    random.seed(11)
    seeds = []
    for nb in (3, 3, 1):
        for _ in range(nb):
            random.randint(0, 9)
        random.getrandbits(32)
        seeds += [random.getrandbits(64), random.getrandbits(64)]
    assert [c[1] for c in on[1]] == seeds and random.getstate() == on[2]
    assert (on[0][0] == 5.0).all() and (on[0][2] == 0.0).all()                    # the unreadable file's row is zeroed last
    proc.set_spec_augment(None)
    only = _epoch(proc, True, monkeypatch)
    assert [c[0] for c in only[1]] == ["channel"] * 3
    proc.set_channel_effects(None)
    again = _epoch(proc, True, monkeypatch)
    assert again[1] == [] and again[2] == control[True][2] and again[3] == control[True][3]


def test_process_audio_file_draws_nothing_more_without_a_config(monkeypatch):
    def run(proc, augment):
        proc.log = []
        calls = _patch(monkeypatch)
        random.seed(5)
        out = proc.process_audio_file("a.wav", augment=augment)
        return out, calls, random.getstate(), list(proc.log)

    proc = _Proc()
    control = {aug: run(proc, aug) for aug in (False, True)}
    assert all(c[1] == [] for c in control.values())
    proc.set_channel_effects(ChannelConfig)
    off = run(proc, False)
    assert off[1] == [] and off[2] == control[False][2] and off[3] == control[False][3]
    proc.set_spec_augment(SpecAugmentConfig)
    on = run(proc, True)
    random.seed(5)
    random.randint(0, 99)
    random.getrandbits(32)
    want = [random.getrandbits(64), random.getrandbits(64)]
    assert [c[0] for c in on[1]] == ["channel", "spec"] and [c[1] for c in on[1]] == want and random.getstate() == on[2]
    assert [x[0] for x in on[3]] == ["load", "augment", "mel"] and on[3][2][1] == 2.0 * 16000
    proc.set_channel_effects(None)
    proc.set_spec_augment(None)
    again = run(proc, True)
    assert again[1] == [] and again[2] == control[True][2] and again[3] == control[True][3]


def test_draw_augment_plan_draws_what_it_drew_before():
    for seed in range(4):
        states = []
        for cfg in (None, ChannelConfig):
            p = pkg.AudioProcessor()
            p.set_channel_effects(cfg)
            random.seed(seed)
            for _ in range(5):
                p.draw_augment_plan()
            states.append(random.getstate())
        assert states[0] == states[1]


def test_restatement_generator_is_batch_independent_and_follows_its_probabilities():
    a, fa = ref.draw_records(SEEDS[2], 259)
    b, fb = ref.draw_records(SEEDS[2], 5)
    assert np.array_equal(a[:5], b) and np.array_equal(fa[:5], fb)                # a clip's record does not depend on n
    assert np.array_equal(~ref.is_identity(a), fa)
    shares = []
    for seed in SEEDS:
        rec, flags = ref.draw_records(seed, 4096)
        assert not flags[:, 5].any()                                              # PEAKS = 3: the fourth peak slot stays the identity
        assert (rec[:, 41:] == 0).all()
        d = rec[:, 40]
        assert ((d == 0) | ((d >= 0.5) & (d <= 3.0))).all()
        touched = ~ref.is_off(rec)
        shares.append(float(touched.mean()))
        # per-section shares among 4096 clips: PROB x the section's own probability, within 4 standard deviations
        for slot, p in ((0, 0.25), (1, 0.25), (2, 0.25), (3, 0.25), (4, 0.25), (6, 0.25), (7, 0.15)):
            assert abs(flags[:, slot].mean() - p) < 4 * (p * (1 - p) / 4096) ** 0.5
        assert abs((d != 0).mean() - 0.1) < 4 * (0.1 * 0.9 / 4096) ** 0.5
        assert all(ref.pole_radius(s) < 1.0 for s in rec[:64, :40].reshape(-1, 5))
    # touched at all: PROB x (1 - the chance that every section and the saturator stay off) = 0.5 x (1 - 0.5^6 x 0.7 x 0.8)
    assert all(abs(s - 0.5 * (1 - 0.5 ** 6 * 0.7 * 0.8)) < 4 * (0.25 / 4096) ** 0.5 for s in shares)
    assert ref.is_off(ref.draw_records(3, 64, prob=0.0)[0]).all()
    full, flags = ref.draw_records(3, 64, prob=1.0, highpass_prob=1.0, low_shelf_prob=1.0, high_shelf_prob=1.0, peaks=4, peak_prob=1.0,
                                   lowpass_prob=1.0, drive_prob=1.0)
    assert flags.all() and (full[:, 40] >= 0.5).all()


def test_restatement_filter_and_saturator():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((3, 2000)).astype(np.float32)
    rec = ops.pack_channel_plans([{}, {"highpass": 20.0}, {"low_shelf": (200.0, 6.0), "peaks": [(1000.0, -6.0, 2.0)], "lowpass": 3400.0, "drive": 2.0}])
    y64, y32 = ref.cascade(x, rec, np.float64), ref.cascade(x, rec, np.float32)
    assert y64.dtype == np.float64 and y32.dtype == np.float32
    assert np.array_equal(y64[0], x[0].astype(np.float64)) and np.array_equal(y32[0], x[0])
    # against the recursion written out sample by sample for one clip
    b0, b1, b2, a1, a2 = rec[1, :5].astype(np.float64)
    y = np.zeros(2002)
    xp = np.concatenate([[0.0, 0.0], x[1].astype(np.float64)])
    for i in range(2000):
        y[i + 2] = b0 * xp[i + 2] + b1 * xp[i + 1] + b2 * xp[i] - a1 * y[i + 1] - a2 * y[i]
    assert np.abs(y[2:] - y64[1]).max() <= 1e-12 * np.abs(y).max()
    err = np.abs(y32.astype(np.float64) - y64).max(axis=1)
    assert err[0] == 0 and (err[1:] > 0).all() and (err[1:] <= 1e-3 * np.abs(y64[1:]).max(axis=1)).all()
    out = ref.apply(x, rec)
    assert np.array_equal(out[:2], y64[:2])                                       # d == 0: the cascade alone
    p = np.abs(y64[2]).max()
    assert abs(np.abs(out[2]).max() - p) <= 2 * np.spacing(p)                     # the saturator keeps the peak
    assert np.array_equal(ref.saturate(-y64[2:], [2.0]), -ref.saturate(y64[2:], [2.0]))
    assert not ref.saturate(np.zeros((1, 8)), [2.0]).any()
    order = np.argsort(y64[2])
    assert (np.diff(out[2][order]) >= 0).all()                                    # monotone
