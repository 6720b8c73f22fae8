"""SpecAugment, everything that needs no GPU: the config validator, the record packing, the C entry points'
refusals before any HIP call, the Meta kernel, the processor's switch, the draws of python `random` with the switch off and on, and the
statistics of the generator's numpy restatement (tests/specaug_ref.py)."""
import random

import numpy as np
import pytest
import torch

import specaug_ref as ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import bank as bankmod
from wakeword_jupyterlab_amd import ops
from wakeword_jupyterlab_amd.config import AugmentationConfig, SpecAugmentConfig, check_spec_augment_config

SEEDS = (0, 1, 2 ** 63 + 12345, 2 ** 64 - 1)


def _cfg(**kw):
    return type("Cfg", (SpecAugmentConfig,), kw)


def test_defaults_and_validator():
    c = SpecAugmentConfig
    assert (c.PROB, c.FREQ_MASKS, c.FREQ_MASK_MAX, c.TIME_MASKS, c.TIME_MASK_MAX_FRACTION, c.FILL) == (0.8, 2, 12, 2, 0.125, "mean")
    assert pkg.SpecAugmentConfig is c
    check_spec_augment_config(c)
    assert [ref.time_max(c.TIME_MASK_MAX_FRACTION, T) for T in (32, 8, 63)] == [4, 1, 7]
    for ok in (_cfg(FILL="min"), _cfg(FILL=-80.0), _cfg(FILL=0), _cfg(PROB=0.0), _cfg(PROB=1), _cfg(FREQ_MASKS=0, TIME_MASKS=4),
               _cfg(FREQ_MASK_MAX=80), _cfg(TIME_MASK_MAX_FRACTION=1.0)):
        check_spec_augment_config(ok)
    for bad in (_cfg(PROB=-0.1), _cfg(PROB=1.5), _cfg(PROB=float("nan")), _cfg(FREQ_MASKS=5), _cfg(TIME_MASKS=5), _cfg(FREQ_MASKS=-1),
                _cfg(FREQ_MASKS=1.5), _cfg(FREQ_MASK_MAX=81), _cfg(FREQ_MASK_MAX=-1), _cfg(TIME_MASK_MAX_FRACTION=1.01),
                _cfg(TIME_MASK_MAX_FRACTION=-0.5), _cfg(FILL="median"), _cfg(FILL=None), _cfg(FILL=float("nan")), _cfg(FILL=True)):
        with pytest.raises(ValueError):
            check_spec_augment_config(bad)
        with pytest.raises(ValueError):
            pkg.AudioProcessor().set_spec_augment(bad)


def test_pack_spec_plans_layout_and_refusals():
    plans = [{}, {"freq": [(0, 3)]}, {"time": [(1, 2), (30, 2)]},
             {"freq": [(1, 2), (3, 4), (5, 6), (70, 10)], "time": [(0, 32), (9, 0), (31, 1), (2, 3)]}]
    rec = ops.pack_spec_plans(plans, 32)
    assert rec.dtype == np.int16 and rec.shape == (4, 16) and rec.flags["C_CONTIGUOUS"]
    assert rec.itemsize * rec.shape[1] == nat.lib.ww_spec_augment_record_bytes() == 32
    assert not rec[0].any()
    assert rec[1].tolist() == [0, 3] + [0] * 14
    assert rec[2].tolist() == [0] * 8 + [1, 2, 30, 2, 0, 0, 0, 0]
    assert rec[3].tolist() == [1, 2, 3, 4, 5, 6, 70, 10, 0, 32, 9, 0, 31, 1, 2, 3]
    m = ref.masks(rec, 32)
    assert not m[0].any() and m[1, :3].all() and not m[1, 3:].any() and m[3].all()
    assert m[2][:, [1, 2, 30, 31]].all() and not m[2][:, [0, 3, 29]].any()
    for bad, T in (([{"freq": [(0, 1)] * 5}], 32), ([{"time": [(0, 1)] * 5}], 32), ([{"freq": [(-1, 2)]}], 32), ([{"freq": [(3, -1)]}], 32),
                   ([{"freq": [(78, 3)]}], 32), ([{"time": [(30, 3)]}], 32), ([{"time": [(0, 9)]}], 8), ([{"time": [(0.5, 1)]}], 8)):
        with pytest.raises(ValueError):
            ops.pack_spec_plans(bad, T)
    assert ops.pack_spec_plans([], 8).shape == (0, 16)


def test_entry_points_refuse_bad_arguments_before_touching_a_device():
    L = nat.lib
    buf = np.zeros(2 * 80 * 8 + 64, np.float32)
    a = (buf.ctypes.data + 15) // 16 * 16                                   # a 16-byte aligned host address: never dereferenced
    rec = a
    good = dict(n=2, width=8, prob=0.5, n_freq=2, freq_max=12, n_time=2, time_max=1, mode=0)

    def apply(mel_in=a, mel_out=a, records=rec, **kw):
        k = dict(good, **kw)
        return L.ww_spec_augment_f32(mel_in, mel_out, k["n"], k["width"], records, 1, k["prob"], k["n_freq"], k["freq_max"], k["n_time"],
                                     k["time_max"], k["mode"], 0.0, None)

    def draw(records=rec, **kw):
        k = dict(good, **kw)
        return L.ww_spec_augment_draw(1, k["n"], k["width"], k["prob"], k["n_freq"], k["freq_max"], k["n_time"], k["time_max"], records, None)

    for call in (apply, draw):
        assert call(width=0) == nat.WW_EUNSUPPORTED and call(width=64) == nat.WW_EUNSUPPORTED
        assert b"width" in L.ww_last_error()
        for kw in (dict(n=-1), dict(n_freq=5), dict(n_time=5), dict(n_freq=-1), dict(freq_max=81), dict(freq_max=-1), dict(time_max=9),
                   dict(time_max=-1), dict(prob=-0.01), dict(prob=1.01), dict(prob=float("nan"))):
            assert call(**kw) == nat.WW_EINVAL, kw
        assert call(n=0, records=None) == nat.WW_OK                         # nothing to do: no launch, no device needed
    assert apply(mode=3) == nat.WW_EINVAL and b"fill mode" in L.ww_last_error()
    assert apply(mode=-1) == nat.WW_EINVAL
    assert apply(n=0, mel_in=None, mel_out=None) == nat.WW_OK
    assert apply(mel_in=None) == nat.WW_EINVAL and apply(mel_out=None) == nat.WW_EINVAL and draw(records=None) == nat.WW_EINVAL
    assert apply(mel_in=a + 4) == nat.WW_EINVAL and apply(records=rec + 2) == nat.WW_EINVAL and draw(records=rec + 2) == nat.WW_EINVAL
    nbytes = 2 * 80 * 8 * 4
    for shift in (16, nbytes - 16):                                         # partial overlap, from either side
        assert apply(mel_out=a + shift) == nat.WW_EINVAL and b"overlap" in L.ww_last_error()
        assert apply(mel_in=a + shift, mel_out=a) == nat.WW_EINVAL
    if not torch.cuda.is_available():                                       # everything in order: only the device is missing
        assert apply() == nat.WW_ENODEVICE                                  # in place
        assert apply(mel_out=a + nbytes) == nat.WW_ENODEVICE                # disjoint
        assert apply(records=None) == nat.WW_ENODEVICE and draw() == nat.WW_ENODEVICE


def test_operator_schema_meta_kernel_and_cpu_refusal():
    ns = torch.ops.wakeword_amd
    assert str(ns.spec_augment.default._schema) == "wakeword_amd::spec_augment(Tensor mel, Tensor records, int fill_mode, float fill_value) -> Tensor"
    for shape in ((3, 1, 80, 33), (5, 80, 8), (0, 1, 80, 63)):
        y = ns.spec_augment(torch.empty(shape, device="meta"), torch.empty((shape[0], 16), dtype=torch.int16, device="meta"), 0, 0.0)
        assert y.shape == shape and y.dtype == torch.float32 and y.device.type == "meta"
    m = lambda *s, **k: torch.empty(*s, device="meta", **k)                 # noqa: E731
    for bad in (lambda: ns.spec_augment(m(3, 1, 80, 64), m(3, 16, dtype=torch.int16), 0, 0.0),
                lambda: ns.spec_augment(m(3, 1, 79, 8), m(3, 16, dtype=torch.int16), 0, 0.0),
                lambda: ns.spec_augment(m(3, 1, 80, 8), m(2, 16, dtype=torch.int16), 0, 0.0),
                lambda: ns.spec_augment(m(3, 1, 80, 8), m(3, 16), 0, 0.0),
                lambda: ns.spec_augment(m(3, 1, 80, 8), m(3, 16, dtype=torch.int16), 3, 0.0)):
        with pytest.raises(RuntimeError):
            bad()
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        ns.spec_augment(torch.zeros(2, 1, 80, 8), torch.zeros(2, 16, dtype=torch.int16), 0, 0.0)


def test_python_wrappers_check_their_arguments():
    rec = torch.zeros(2, 16, dtype=torch.int16)
    with pytest.raises(RuntimeError):
        ops.spec_augment(torch.zeros(2, 1, 80, 8), rec)                     # a CPU tensor
    with pytest.raises(RuntimeError):
        ops.spec_augment_records(1, 4, 8, device="cpu")
    with pytest.raises(NotImplementedError):
        ops.spec_augment_records(1, 4, 64, device="cuda")
    with pytest.raises(ValueError):
        ops.spec_augment_records(1, 4, 8, _cfg(FREQ_MASKS=9), device="cuda")


def test_switch_is_off_by_default_and_mirrors_the_other_banks():
    p = pkg.AudioProcessor()
    assert p.spec_augment is None
    assert p.set_spec_augment(SpecAugmentConfig) is SpecAugmentConfig and p.spec_augment is SpecAugmentConfig
    assert p.set_spec_augment(None) is None and p.spec_augment is None


def _reference_draws(config=AugmentationConfig, sr=16000, n=16000):
    """AudioProcessor.draw_augment_plan's draws without banks, restated: what the parent commit consumes of python `random`."""
    if random.random() < config.AUGMENTATION_PROB:
        random.uniform(-config.TIME_SHIFT_MAX, config.TIME_SHIFT_MAX)
    if random.random() < config.AUGMENTATION_PROB:
        random.uniform(-config.PITCH_SHIFT_MAX, config.PITCH_SHIFT_MAX)
    if random.random() < config.AUGMENTATION_PROB:
        rate = random.uniform(config.SPEED_CHANGE_MIN, config.SPEED_CHANGE_MAX)
        if int(round(n / rate)) > n:
            random.randint(0, int(round(n / rate)) - n)
    if random.random() < config.AUGMENTATION_PROB:
        random.getrandbits(32)


def test_draw_augment_plan_draws_what_it_drew_before():
    for seed in range(6):
        random.seed(seed)
        for _ in range(5):
            _reference_draws()
        want = random.getstate()
        for cfg in (None, SpecAugmentConfig):
            p = pkg.AudioProcessor()
            p.set_spec_augment(cfg)
            random.seed(seed)
            for _ in range(5):
                p.draw_augment_plan()
            assert random.getstate() == want


class _Proc(pkg.AudioProcessor):
    """The processor's device work replaced by host stand-ins: the loaders' own logic (what is drawn, what is called, in which order) runs."""

    def augment_batch(self, pcm, plans=None, config=AugmentationConfig):
        self.log.append(("augment", random.getrandbits(32)))
        return pcm

    def mel_batch(self, pcm, normalize=True):
        self.log.append(("mel",))
        return torch.ones(pcm.shape[0], 1, 80, 32)


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


def _epoch(proc, augment, monkeypatch):
    proc.log = []
    calls = []

    def fake(mel, records=None, *, seed=None, config=None, out=None):
        calls.append((seed, config, out is mel))
        mel.fill_(5.0)
        return mel
    monkeypatch.setattr(ops, "spec_augment", fake)
    random.seed(11)
    batches = [d.clone() for d, _ in bankmod.BankLoader(_Bank(proc), 3, augment=augment)]
    return batches, calls, random.getstate(), list(proc.log)


def test_bank_loader_host_logic_draws_one_seed_per_augmented_batch_and_nothing_otherwise(monkeypatch):
    proc = _Proc()
    control = {aug: _epoch(proc, aug, monkeypatch) for aug in (False, True)}       # no config: the loader as it was
    assert all(c[1] == [] for c in control.values())
    proc.set_spec_augment(SpecAugmentConfig)
    off = _epoch(proc, False, monkeypatch)
    assert off[1] == [] and off[2] == control[False][2] and off[3] == control[False][3]
    assert all(torch.equal(x, y) for x, y in zip(off[0], control[False][0]))
    on = _epoch(proc, True, monkeypatch)
    assert len(on[1]) == 3 and all(cfg is SpecAugmentConfig and inplace for _, cfg, inplace in on[1])
    assert [x[0] for x in on[3]] == [x[0] for x in control[True][3]]              # the same calls in the same order
    # the replay: starts, augment_batch's draw, then ONE 64-bit seed per batch
    random.seed(11)
    seeds = []
    for nb in (3, 3, 1):
        for _ in range(nb):
            random.randint(0, 9)
        random.getrandbits(32)
        seeds.append(random.getrandbits(64))
    assert [s for s, _, _ in on[1]] == seeds and random.getstate() == on[2]
    assert (on[0][0] == 5.0).all() and (on[0][2] == 0.0).all()                    # the unreadable file's row is zeroed last
    proc.set_spec_augment(None)
    again = _epoch(proc, True, monkeypatch)
    assert again[1] == [] and again[2] == control[True][2]


def test_restatement_statistics():
    """The figures the generator's specification was checked with: 4096 clips, default config."""
    shares, least = [], 10 ** 9
    for seed in SEEDS:
        for T in (8, 32, 63):
            share, counts, in_bounds = ref.statistics(seed, 4096, T)
            assert in_bounds and counts.shape == (13,)
            shares.append(share)
            least = min(least, int(counts.min()))
    assert (round(min(shares), 4), round(max(shares), 4)) == (0.7935, 0.8079) and least >= 449    # 3250 and 3309 of 4096 clips
    a, b = ref.draw_records(SEEDS[2], 259, 32), ref.draw_records(SEEDS[2], 5, 32)
    assert np.array_equal(a[:5], b)                                               # a clip's record does not depend on n
    assert not ref.draw_records(3, 64, 32, prob=0.0).any()
    full = ref.draw_records(3, 64, 32, prob=1.0, n_freq=4, n_time=4, freq_max=80, t_max=32).astype(int)
    assert (full[:, 0:8:2] + full[:, 1:8:2] <= 80).all() and (full[:, 8:16:2] + full[:, 9:16:2] <= 32).all()


def test_restatement_masking():
    rng = np.random.default_rng(0)
    mel = (-80 * rng.random((3, 80, 8))).astype(np.float32)
    rec = ops.pack_spec_plans([{}, {"freq": [(79, 1)], "time": [(0, 1)]}, {"time": [(0, 8)]}], 8)
    for fill in ("mean", "min", -80.0):
        out = ref.apply(mel, rec, fill)
        assert np.array_equal(out[0], mel[0])
        f = np.float32(ref.fills(mel, fill)[1])
        assert (out[1, 79] == f).all() and (out[1, :, 0] == f).all() and np.array_equal(out[1, :79, 1:], mel[1, :79, 1:])
        assert (out[2] == np.float32(ref.fills(mel, fill)[2])).all()
    assert ref.fills(mel, "min")[1] == mel[1].min() and abs(ref.fills(mel, "mean")[1] - mel[1].astype(np.float64).mean()) == 0
