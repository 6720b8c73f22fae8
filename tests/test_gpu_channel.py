"""Microphone-channel augmentation on the MI355X against its numpy restatement (tests/channel_ref.py).

The filter's bound is the project's rule for float32 kernels (oracle/train_oracle.py, ratio_f32): per clip
    max |out - ref64| <= 4 max |ref32 - ref64| + 2^-22 max |ref64|
with ref64 the sequential float64 recursion on the record's float32 coefficients and ref32 the same recursion with every operation
rounded to float32; the test asserts max |ref32 - ref64| <= 1e-3 max |ref64| for every clip it uses, so that the yardstick means
something.  The records' bound is one float32 ulp of the float64 coefficient rounded to float32 (device and host libm may differ in the last
bits of float64 sin / cos / pow, which can move one float32 rounding).  Shapes: B <= 70, N in {4000, 4003, 15920, 16000, 16383}; the
references of a shape are computed once and shared."""
import os
import random

import numpy as np
import pytest
import torch

import channel_ref as ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import ops, synth
from wakeword_jupyterlab_amd.config import ChannelConfig, SpecAugmentConfig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LENGTHS = (4000, 4003, 15920, 16000, 16383)    # the shortest clip; no multiple of 256; 1 s minus a bit; the 1 s clip; the longest clip
SEEDS = (0, 1, 2 ** 63 + 12345, 2 ** 64 - 1)
ALL_ON = {"highpass": 20.0, "low_shelf": (150.0, 5.0), "peaks": [(100.0, 6.0, 4.0), (700.0, -4.0, 1.0), (2200.0, 5.0, 0.7), (5000.0, -6.0, 2.0)],
          "high_shelf": (3000.0, -5.0), "lowpass": 3400.0}


def _cfg(**kw):
    return type("Cfg", (ChannelConfig,), kw)


EVERYTHING = _cfg(PROB=1.0, HIGHPASS_PROB=1.0, LOW_SHELF_PROB=1.0, HIGH_SHELF_PROB=1.0, PEAKS=4, PEAK_PROB=1.0, LOWPASS_PROB=1.0, DRIVE_PROB=1.0)


def _signals(N):
    """float32 [4, N]: seeded noise, a unit impulse, a step, a 1 kHz sine."""
    x = np.zeros((4, N), np.float32)
    x[0] = (2.0 * synth.uniform01(77 + N, 1, N).reshape(N) - 1.0).astype(np.float32)
    x[1, 0] = 1.0
    x[2, N // 3:] = 0.75
    x[3] = (0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(N) / 16000.0)).astype(np.float32)
    return x


_CASES = {}


def _case(N):
    """(x [B, N], records [B, 48], ref64, ref32) -- built once per length and left unchanged.  Rows: the four signals under records the
    device drew (default config, then every section on), then under explicit records with all 8 sections on, without and with drive."""
    if N not in _CASES:
        n_default = 54 if N == 16000 else 8
        drawn = torch.cat([ops.channel_records(SEEDS[2], n_default, device=DEV), ops.channel_records(SEEDS[1], 8, EVERYTHING, device=DEV)])
        explicit = ops.pack_channel_plans([ALL_ON] * 4 + [dict(ALL_ON, drive=2.0)] * 4)
        rec = np.concatenate([drawn.cpu().numpy(), explicit])
        x = np.tile(_signals(N), (rec.shape[0] // 4 + 1, 1))[:rec.shape[0]]
        r64, r32 = ref.apply(x, rec, np.float64), ref.apply(x, rec, np.float32)
        for a in (x, rec, r64, r32):
            a.setflags(write=False)
        _CASES[N] = (x, rec, r64, r32)
    return _CASES[N]


def _bounds(r64, r32):
    """(the bound per clip, the yardstick's own error, the reference's peak)."""
    peak = np.abs(r64).max(axis=-1)
    own = np.abs(r32.astype(np.float64) - r64).max(axis=-1)
    return 4.0 * own + 2.0 ** -22 * peak, own, peak


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _ulps(a, b):
    """Distance in float32 ulps between two float32 arrays of finite values."""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ---- 1. records -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_drawn_records_equal_the_restatement(seed):
    for cfg in (ChannelConfig, EVERYTHING, _cfg(HIGHPASS_HZ=(20.0, 20.0), PEAK_Q=(4.0, 4.0), PEAK_HZ=(100.0, 100.0), PROB=1.0, PEAKS=1)):
        got_t = ops.channel_records(seed, 70, cfg, device=DEV)
        assert got_t.dtype == torch.float32 and got_t.shape == (70, 48)
        got = got_t.cpu().numpy()
        want, flags = ref.draw_records(seed, 70, **ref.config_of(cfg))
        assert np.array_equal(~ref.is_identity(got), flags)                       # which slots are identity, exactly
        assert np.array_equal(got[:, 40] != 0, want[:, 40] != 0) and (got[:, 41:] == 0).all()
        worst = int(_ulps(got, want).max())
        print(f"seed {seed} {cfg.__name__}: largest record distance {worst} ulp")
        assert worst <= 1
        assert torch.equal(ops.channel_records(seed, 5, cfg, device=DEV), got_t[:5])      # a clip's record does not depend on B
    assert ref.is_off(ops.channel_records(seed, 64, _cfg(PROB=0.0), device=DEV).cpu().numpy()).all()
    assert ops.channel_records(seed, 0, device=DEV).shape == (0, 48)


# ---- 2. the filter against float64 on its own input -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", LENGTHS)
def test_filter_against_float64(N):
    x, rec, r64, r32 = _case(N)
    bound, own, peak = _bounds(r64, r32)
    assert (own <= 1e-3 * peak).all(), "the float32 yardstick is not usable for these clips"
    out = ops.channel_effects(_dev(x), _dev(rec))
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    err = np.abs(got - r64).max(axis=1)
    w = int(np.argmax(err / bound))
    print(f"N {N}: worst clip {w}: err {err[w]:.3e}, bound {bound[w]:.3e} (yardstick {own[w]:.3e}, peak {peak[w]:.3e}); "
          f"largest err / peak {np.max(err / peak):.3e}, largest yardstick / peak {np.max(own / peak):.3e}")
    assert np.isfinite(got).all() and (err <= bound).all(), (w, err[w], bound[w])
    off = ref.is_off(rec)
    assert np.array_equal(out.cpu().numpy()[off].view(np.int32), x[off].view(np.int32))    # out of place: copied through bit for bit
    # the compiled operator is the same launch
    assert torch.equal(torch.ops.wakeword_amd.channel_effects(_dev(x), _dev(rec)), out)


# ---- 3. an independent check: the steady-state amplitude of a sine is |H| -------------------------------------------------------------
@pytest.mark.parametrize("N", (4000, 16383))
def test_sine_amplitude_equals_the_frequency_response(N):
    """The amplitude over the last quarter of the clip, from a least-squares fit of sin and cos at f, against |H(e^{jw})| evaluated in
    float64 from the record's coefficients.  Bound: 2 (e_kernel + e_input) + transient.  A least-squares fit onto {sin, cos} over n samples
    moves the amplitude by at most 2 max |e| for an error e (each coefficient by at most sqrt(2) max |e|).  e_kernel is the bound of item
    2; e_input = 2^-25 |h|_1 is what rounding the sine to float32 (|x| <= 0.5) can add at the output.  The transient is a sum of 2 x 6
    modes c p^n; with |c| <= 1e3 (generous: these sections are well separated, their residues are O(1)) it is at most 1.2e4 r^n0 at
    the window's start n0 = 3 N / 4, r the largest pole radius: zero to every digit here, r < 0.95."""
    plan = {"highpass": 300.0, "low_shelf": (400.0, 4.0), "peaks": [(1000.0, 6.0, 1.0), (2500.0, -5.0, 1.5)], "high_shelf": (3000.0, -4.0),
            "lowpass": 6000.0}
    rec = ops.pack_channel_plans([plan] * 3)
    sections = rec[0, :40].reshape(8, 5)
    r = ref.pole_radius(sections)
    assert r < 0.95
    n = np.arange(N)
    freqs = (100.0, 1000.0, 5000.0)
    x = np.stack([(0.5 * np.sin(2 * np.pi * f * n / 16000.0)).astype(np.float32) for f in freqs])
    r64, r32 = ref.apply(x, rec, np.float64), ref.apply(x, rec, np.float32)
    e_kernel, own, peak = _bounds(r64, r32)
    assert (own <= 1e-3 * peak).all()
    impulse = np.zeros((1, N), np.float32)
    impulse[0, 0] = 1.0
    h1 = np.abs(ref.cascade(impulse, rec[:1])).sum()
    got = ops.channel_effects(_dev(x), _dev(rec)).cpu().numpy().astype(np.float64)
    n0 = 3 * N // 4
    for k, f in enumerate(freqs):
        basis = np.stack([np.sin(2 * np.pi * f * n[n0:] / 16000.0), np.cos(2 * np.pi * f * n[n0:] / 16000.0)], axis=1)
        coef, *_ = np.linalg.lstsq(basis, got[k, n0:], rcond=None)
        amp, want = float(np.hypot(*coef)), 0.5 * ref.response(sections, f)
        bound = 2.0 * (e_kernel[k] + 2.0 ** -25 * h1) + 1.2e4 * r ** n0
        print(f"N {N} f {f}: amplitude {amp:.9f}, 0.5 |H| {want:.9f}, difference {abs(amp - want):.3e}, bound {bound:.3e}")
        assert abs(amp - want) <= bound


# ---- 4. the saturator -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (4003, 16000))
def test_saturator(N):
    noise = _signals(N)[0]
    x = np.stack([noise, -noise, noise, noise, np.zeros(N, np.float32), noise])
    plans = [{"drive": 0.5}, {"drive": 0.5}, {"drive": 3.0}, {"drive": 8.0}, {"drive": 3.0}, {}]
    out = ops.channel_effects(_dev(x), _dev(ops.pack_channel_plans(plans))).cpu().numpy()
    p = np.float32(np.abs(noise).max())
    for row in (0, 2, 3):                                                         # identity sections: the saturator's input is the clip
        assert _ulps(np.abs(out[row]).max(), p) <= 2
        order = np.argsort(noise, kind="stable")
        assert (np.diff(out[row][order]) >= 0).all()                              # monotone in the input
        assert (np.sign(out[row]) == np.sign(noise)).all()
        d = plans[row]["drive"]
        want = float(p) * np.tanh(d * noise.astype(np.float64) / float(p)) / np.tanh(d)
        assert (_ulps(out[row], want.astype(np.float32)) <= 1).all()
    assert np.array_equal(out[1].view(np.int32), (-out[0]).view(np.int32))        # odd-symmetric
    assert not out[4].any() and not np.isnan(out[4]).any()                        # an all-zero clip gives all zeros
    assert np.array_equal(out[5].view(np.int32), noise.view(np.int32))
    # behind a cascade: d == 0 is the cascade alone, bit for bit, and the drive keeps the cascade's peak
    rec = ops.pack_channel_plans([ALL_ON, dict(ALL_ON, drive=0.0), dict(ALL_ON, drive=2.0)])
    y = ops.channel_effects(_dev(np.stack([noise] * 3)), _dev(rec)).cpu().numpy()
    assert np.array_equal(y[0].view(np.int32), y[1].view(np.int32))
    py = np.abs(y[0]).max()
    assert _ulps(np.abs(y[2]).max(), py) <= 2
    want = float(py) * np.tanh(2.0 * y[0].astype(np.float64) / float(py)) / np.tanh(2.0)
    assert (_ulps(y[2], want.astype(np.float32)) <= 1).all()


# ---- 5. structure ---------------------------------------------------------------------------------------------------------------------
def test_off_records_in_place_are_never_written_and_out_of_place_leaves_the_input():
    x, rec, _, _ = _case(16000)
    off = ref.is_off(rec)
    assert off.any() and not off.all()
    poison = np.float32(np.nan).view(np.int32) | 0x12345
    buf = np.array(x)
    buf.view(np.int32)[off] = poison                                              # NaNs with a payload: arithmetic would not keep them
    t = _dev(buf)
    src = t.clone()
    want = ops.channel_effects(src, _dev(rec))
    assert torch.equal(src.view(torch.int32), t.view(torch.int32))                # out of place leaves the input untouched
    assert ops.channel_effects(t, _dev(rec), out=t) is t
    got = t.cpu().numpy()
    assert (got.view(np.int32)[off] == poison).all()
    assert np.array_equal(got.view(np.int32), want.cpu().numpy().view(np.int32))  # in place = out of place


def test_rows_do_not_depend_on_the_batch_or_their_position_and_runs_repeat():
    x, rec, _, _ = _case(16000)
    B = x.shape[0]
    assert B == 70
    full = ops.channel_effects(_dev(x), _dev(rec))
    assert torch.equal(ops.channel_effects(_dev(x), _dev(rec)), full)             # two runs, the same bits
    perm = np.random.default_rng(3).permutation(B)
    moved = ops.channel_effects(_dev(x[perm]), _dev(rec[perm]))
    assert torch.equal(moved, full[torch.from_numpy(perm).to(DEV)])
    rows = [69, 3, 62, 17, 40]
    few = ops.channel_effects(_dev(x[rows]), _dev(rec[rows]))
    assert torch.equal(few, full[rows])
    one = ops.channel_effects(_dev(x[62:63]), _dev(rec[62:63]))
    assert torch.equal(one, full[62:63])


@pytest.mark.parametrize("N", (4003, 16000))
def test_seed_form_equals_records_form(N):
    x = _dev(np.tile(_signals(N), (18, 1))[:70])
    for seed, cfg in ((SEEDS[1], ChannelConfig), (SEEDS[3], EVERYTHING)):
        rec = ops.channel_records(seed, 70, cfg, device=DEV)
        a, b = ops.channel_effects(x, seed=seed, config=cfg), ops.channel_effects(x, rec)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not torch.equal(a, x)
        y = x.clone()
        ops.channel_effects(y, seed=seed, config=cfg, out=y)
        assert torch.equal(y.view(torch.int32), a.view(torch.int32))
        off = torch.from_numpy(ref.is_off(rec.cpu().numpy())).to(DEV)
        assert torch.equal(a[off].view(torch.int32), x[off].view(torch.int32))
    assert ops.channel_effects(torch.zeros(0, N, device=DEV), seed=3).shape == (0, N)


def test_wrapper_refusals_on_the_device():
    pcm = torch.zeros(2, 4000, device=DEV)
    rec = torch.zeros(2, 48, device=DEV)
    for bad in (lambda: ops.channel_effects(pcm, rec, seed=1), lambda: ops.channel_effects(pcm), lambda: ops.channel_effects(pcm.double(), rec),
                lambda: ops.channel_effects(pcm, rec[:1]), lambda: ops.channel_effects(pcm, rec.double()),
                lambda: ops.channel_effects(pcm, rec, out=torch.zeros(2, 4001, device=DEV)),
                lambda: ops.channel_effects(torch.zeros(4000, 2, device=DEV).t(), rec), lambda: ops.channel_effects(pcm, seed=1, config=_cfg(PEAKS=5))):
        with pytest.raises(ValueError):
            bad()
    for n in (3999, 16384, 32000):
        with pytest.raises(NotImplementedError):
            ops.channel_effects(torch.zeros(2, n, device=DEV), rec)
    big = torch.zeros(3 * 4000, device=DEV)                                       # partially overlapping in / out: refused by the library
    with pytest.raises(RuntimeError, match="overlap"):
        ops.channel_effects(big[:8000].view(2, 4000), rec, out=big[2000:10000].view(2, 4000))


# ---- 6. non-finite input --------------------------------------------------------------------------------------------------------------
def test_a_nan_or_an_inf_stays_in_its_row_and_behind_its_sample():
    """One run: the damaged rows (all 8 sections on, no drive) are right up to the bad sample, every other row has the bits it has in the
    undamaged batch."""
    N, k = 4003, 2500                                                             # sample 2500: inside thread 156's chunk of 16
    x, rec, r64, r32 = _case(N)
    rows = {16: np.float32(np.nan), 18: np.float32(np.inf)}                       # explicit all-on records, d == 0: the noise, the step
    assert all(not ref.is_identity(rec[r:r + 1]).any() and rec[r, 40] == 0 for r in rows)
    clean = ops.channel_effects(_dev(x), _dev(rec)).cpu().numpy()
    bad = np.array(x)
    for r, v in rows.items():
        bad[r, k] = v
    got = ops.channel_effects(_dev(bad), _dev(rec))
    torch.cuda.synchronize()                                                      # the call returns
    got = got.cpu().numpy()
    others = np.array([r not in rows for r in range(x.shape[0])])
    assert np.array_equal(got[others].view(np.int32), clean[others].view(np.int32))
    for r in rows:
        bound, own, peak = _bounds(r64[r, :k], r32[r, :k])
        assert own <= 1e-3 * peak
        err = np.abs(got[r, :k].astype(np.float64) - r64[r, :k]).max()
        print(f"row {r}: err before the bad sample {err:.3e}, bound {bound:.3e}")
        assert err <= bound
        assert not np.isfinite(got[r, k])


# ---- 7. loaders: a dozen synthetic one-second files, batch 5 --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("channel")
    clips = synth.make_clips(0, 12)
    paths = []
    for i in range(12):
        paths.append(os.path.join(d, f"clip_{i:02d}.wav"))
        synth.write_wav16(paths[-1], clips[i])
    return paths


ON = _cfg(PROB=1.0)


def _dataset(files, channel, spec=None, augment=True):
    proc = pkg.AudioProcessor(device=DEV)
    proc.set_channel_effects(channel)
    proc.set_spec_augment(spec)
    return pkg.WakewordDataset(files[:6], files[6:], proc, augment=augment, verbose=False)


def _run(loader, seed=3):
    random.seed(seed)
    torch.manual_seed(seed)
    out = [(d.clone(), t.clone()) for d, t in loader]
    torch.cuda.synchronize()
    return out, random.getstate()


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(p[0].view(torch.int32), q[0].view(torch.int32)) and torch.equal(p[1], q[1]) for p, q in zip(a, b))


@pytest.mark.parametrize("kind", ("files", "bank"))
def test_loaders_equal_a_hand_written_chain(files, kind):
    ds = _dataset(files, ON, SpecAugmentConfig)
    proc = ds.processor
    make = (lambda: ds.loader(5)) if kind == "files" else (lambda bank=ds.cache(): bank.loader(5, augment=True))
    got, state = _run(make())
    assert [d.shape[0] for d, _ in got] == [5, 5, 2]
    again, again_state = _run(make())
    assert _same(got, again) and state == again_state                             # a seeded epoch repeats bit for bit
    random.seed(3)
    torch.manual_seed(3)
    changed = False
    for k, s in enumerate(range(0, 12, 5)):
        pcm, ok = proc.load_clips_gpu(ds.files[s:s + 5])
        assert ok.all()
        pcm = proc.augment_batch(pcm)
        plain = pcm.clone()
        seed = random.getrandbits(64)                                             # that draw: after augment_batch's plans
        assert proc.channel_effects_batch(pcm, seed=seed, inplace=True) is pcm
        changed |= not torch.equal(plain, pcm)
        assert torch.equal(pcm, ops.channel_effects(plain, ops.channel_records(seed, pcm.shape[0], ON, device=DEV)))
        mel = proc.mel_batch(pcm, normalize=False)
        proc.spec_augment_batch(mel, inplace=True)                                # draws its own seed next
        assert torch.equal(got[k][0].view(torch.int32), mel.view(torch.int32))
    assert changed and random.getstate() == state


@pytest.mark.parametrize("kind", ("files", "bank"))
def test_unset_and_validation_loaders_are_untouched(files, kind):
    def make(channel, augment, touch=False):
        ds = _dataset(files, channel, augment=augment)
        if touch:
            ds.processor.set_channel_effects(ON)
            ds.processor.set_channel_effects(None)
        return ds.loader(5) if kind == "files" else ds.cache().loader(5, augment=augment)
    control, control_state = _run(make(None, False))
    got, state = _run(make(ON, False))                                            # a validation loader with a config set
    assert state == control_state and _same(got, control)
    aug_control, aug_control_state = _run(make(None, True))
    unset, unset_state = _run(make(None, True, touch=True))                       # set, then unset: the loader as it was
    assert unset_state == aug_control_state and _same(unset, aug_control)
    aug, aug_state = _run(make(ON, True))                                         # and set: one 64-bit draw per batch, other data
    assert aug_state != aug_control_state and torch.equal(aug[0][1], aug_control[0][1]) and not torch.equal(aug[0][0], aug_control[0][0])


def test_process_audio_file_and_items_follow_the_same_order(files):
    ds = _dataset(files, ON, SpecAugmentConfig)
    proc = ds.processor
    for seed in range(3):
        random.seed(seed)
        got = proc.process_audio_file(files[seed], augment=True)
        state = random.getstate()
        assert got.shape == (80, 32) and got.dtype == np.float32
        random.seed(seed)                                                         # by hand: crop, plan, channel seed, log-mel, masking seed
        pcm, _ = proc.load_clips_gpu([files[seed]])
        pcm = proc.augment_batch(pcm)
        proc.channel_effects_batch(pcm, seed=random.getrandbits(64), inplace=True)
        mel = proc.mel_batch(pcm, normalize=False)
        proc.spec_augment_batch(mel, inplace=True)
        assert random.getstate() == state
        assert np.array_equal(got.view(np.int32), mel[0, 0].cpu().numpy().view(np.int32))
        random.seed(seed)
        item, label = ds[seed]
        assert random.getstate() == state and int(label) == 1
        assert np.array_equal(item[0].numpy().view(np.int32), got.view(np.int32))
    random.seed(0)
    assert np.array_equal(proc.process_audio_file(files[0], augment=False),
                          pkg.AudioProcessor(device=DEV).process_audio_file(files[0], augment=False))
