"""SpecAugment on the MI355X against its numpy restatement (tests/specaug_ref.py): explicit plans at every
width class and fill mode (unmasked bits, exact minimum and constant fills, the mean within one float32 ulp of the float64 mean, in place
against out of place, guard rows), the records drawn on the device against the generator's restatement bit for bit, and the loaders with
the switch on against a hand-written loop.

The mean's bound is derived, not measured: the kernel adds 80 T <= 5040 floats in double, which leaves a relative error of at most
5040 * 2^-53 in the sum, far below half a float32 ulp; the one rounding to float32 then lands within one float32 ulp of the exact mean."""
import os
import random

import numpy as np
import pytest
import torch

import specaug_ref as ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import ops, synth
from wakeword_jupyterlab_amd.config import SpecAugmentConfig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
WIDTHS = (1, 8, 31, 32, 33, 63)           # one frame; 0.25 s; the 1 s image and its neighbours (a float4 straddles rows); 2 s
BATCHES = (1, 5, 259)                     # 259: more clips than CUs, no multiple of the clips per workgroup
FILLS = ("mean", "min", -37.25)
SEEDS = (0, 1, 2 ** 63 + 12345, 2 ** 64 - 1)
SENTINEL = 12345.5


def _cfg(**kw):
    return type("Cfg", (SpecAugmentConfig,), kw)


def _plans(B, T):
    """The eight kinds of the issue's list, cycling over the clips of a batch."""
    def t(s, w):                           # a frame block pulled inside 0 .. T
        s = min(s, T - 1)
        return s, min(w, T - s)
    w = max(1, T // 8)
    kinds = [{},
             {"freq": [(0, 5)]},
             {"freq": [(73, 7)]},
             {"time": [(0, w), (T - w, w)]},
             {"freq": [(10, 8), (14, 8), (16, 2), (40, 12)], "time": [t(0, 2), t(1, 2), t(1, 1), t(T // 2, 3)]},
             {"time": [(0, T)]},
             {"freq": [(0, 80)]},
             {"freq": [(0, 1), (79, 1), (37, 1)], "time": [(0, 1), (T - 1, 1)]}]
    return [kinds[i % len(kinds)] for i in range(B)]


_CASES = {}


def _case(B, T):
    """(mel float32 [B, 80, T] in log-mel's range, records int16 [B, 16], masks) -- built once per shape and left unchanged."""
    if (B, T) not in _CASES:
        mel = (-80.0 * synth.uniform01(1000 + T, B, B * 80 * T)).astype(np.float32).reshape(B, 80, T)
        rec = ops.pack_spec_plans(_plans(B, T), T)
        for a in (mel, rec):
            a.setflags(write=False)
        _CASES[(B, T)] = (mel, rec, ref.masks(rec, T))
    return _CASES[(B, T)]


def _guarded(mel):
    """mel [B, 80, T] inside a larger device buffer with one sentinel clip before and one after: (buffer, the [B, 1, 80, T] view)."""
    B, _, T = mel.shape
    buf = torch.full(((B + 2) * 80 * T,), SENTINEL, device=DEV)
    view = buf[80 * T:(B + 1) * 80 * T].view(B, 1, 80, T)
    view.copy_(torch.from_numpy(np.array(mel)).view(B, 1, 80, T))
    return buf, view


def _guards_intact(buf, B, T):
    return bool((buf[:80 * T] == SENTINEL).all() and (buf[(B + 1) * 80 * T:] == SENTINEL).all())


@pytest.mark.parametrize("fill", FILLS, ids=lambda f: str(f))
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("T", WIDTHS)
def test_explicit_plans(T, B, fill):
    mel, rec, m = _case(B, T)
    cfg = _cfg(FILL=fill)
    records = torch.from_numpy(np.array(rec)).to(DEV)
    src_buf, src = _guarded(mel)
    out_buf, out = _guarded(np.zeros_like(mel))
    got_t = ops.spec_augment(src, records, config=cfg, out=out)
    assert got_t is out and _guards_intact(out_buf, B, T) and _guards_intact(src_buf, B, T)
    assert torch.equal(src.cpu().view(B, 80, T), torch.from_numpy(np.array(mel)))          # out of place: the input is left alone
    got = out.cpu().numpy().reshape(B, 80, T)
    # unmasked positions: the input's bits
    assert np.array_equal(got.view(np.int32)[~m], mel.view(np.int32)[~m])
    if fill == "mean":
        exact = ref.fills(mel, "mean")
        for c in range(B):
            v = got[c][m[c]]
            if v.size:
                assert (v.view(np.int32) == v.view(np.int32)[0]).all(), "one fill value per clip"
                assert abs(float(v[0]) - exact[c]) <= np.spacing(np.float32(abs(exact[c]))), (c, float(v[0]), exact[c])
    else:
        assert np.array_equal(got.view(np.int32), ref.apply(mel, rec, fill).view(np.int32))
    # the same call twice; a fresh output tensor; in place
    again = ops.spec_augment(src, records, config=cfg)
    assert torch.equal(again, out) and again.data_ptr() != src.data_ptr()
    same = ops.spec_augment(src, records, config=cfg, out=src)
    assert same is src and torch.equal(src, out) and _guards_intact(src_buf, B, T)
    if B == 5:                                                                             # the 3-d form, and the compiled operator
        flat = ops.spec_augment(torch.from_numpy(np.array(mel)).to(DEV), records, config=cfg)
        assert flat.shape == (B, 80, T) and torch.equal(flat.view(B, 1, 80, T), out)
        mode, value = (0, 0.0) if fill == "mean" else (1, 0.0) if fill == "min" else (2, float(fill))
        op = torch.ops.wakeword_amd.spec_augment(torch.from_numpy(np.array(mel)).to(DEV).view(B, 1, 80, T), records, mode, value)
        assert torch.equal(op, out)


def test_in_place_leaves_a_clip_without_masks_alone_and_a_constant_fill_reads_nothing():
    """A NaN clip without masks stays as it is in place; under a constant fill NaNs under the masks do not spread."""
    T, B = 32, 3
    mel = torch.full((B, 1, 80, T), float("nan"), device=DEV)
    records = torch.from_numpy(ops.pack_spec_plans([{}, {"freq": [(3, 2)]}, {"time": [(0, T)]}], T)).to(DEV)
    ops.spec_augment(mel, records, config=_cfg(FILL=-80.0), out=mel)
    got = mel.cpu().numpy().reshape(B, 80, T)
    assert np.isnan(got[0]).all() and (got[1, 3:5] == -80.0).all() and np.isnan(got[1, :3]).all() and np.isnan(got[1, 5:]).all()
    assert (got[2] == -80.0).all()


def test_wrapper_refusals_on_the_device():
    mel = torch.zeros(2, 1, 80, 8, device=DEV)
    rec = torch.zeros(2, 16, dtype=torch.int16, device=DEV)
    for bad in (lambda: ops.spec_augment(mel, rec, seed=1), lambda: ops.spec_augment(mel), lambda: ops.spec_augment(mel.double(), rec),
                lambda: ops.spec_augment(torch.zeros(2, 1, 79, 8, device=DEV), rec), lambda: ops.spec_augment(mel, rec[:1]),
                lambda: ops.spec_augment(mel, rec.int()), lambda: ops.spec_augment(mel, rec, out=torch.zeros(2, 1, 80, 9, device=DEV)),
                lambda: ops.spec_augment(mel.transpose(2, 3).contiguous().transpose(2, 3), rec)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(NotImplementedError):
        ops.spec_augment(torch.zeros(2, 1, 80, 64, device=DEV), rec)
    with pytest.raises(RuntimeError):
        ops.spec_augment(mel.cpu(), rec)
    big = torch.zeros(3 * 80 * 8, device=DEV)                                               # partially overlapping in / out: refused by the library
    with pytest.raises(RuntimeError, match="overlap"):
        ops.spec_augment(big[:2 * 640].view(2, 1, 80, 8), rec, out=big[320:320 + 2 * 640].view(2, 1, 80, 8))
    assert ops.spec_augment(torch.zeros(0, 1, 80, 8, device=DEV), seed=3).shape == (0, 1, 80, 8)


@pytest.mark.parametrize("T", (8, 32, 63))
def test_drawn_records_equal_the_restatement(T):
    for seed in SEEDS:
        got = ops.spec_augment_records(seed, 259, T, device=DEV)
        assert got.dtype == torch.int16 and got.shape == (259, 16)
        assert np.array_equal(got.cpu().numpy(), ref.draw_records(seed, 259, T))
        assert torch.equal(ops.spec_augment_records(seed, 5, T, device=DEV), got[:5])      # a clip's record does not depend on n
    cfg = _cfg(PROB=1.0, FREQ_MASKS=4, FREQ_MASK_MAX=80, TIME_MASKS=4, TIME_MASK_MAX_FRACTION=1.0)
    got = ops.spec_augment_records(SEEDS[2], 259, T, cfg, device=DEV).cpu().numpy()
    assert np.array_equal(got, ref.draw_records(SEEDS[2], 259, T, prob=1.0, n_freq=4, freq_max=80, n_time=4, t_max=T))
    assert not ops.spec_augment_records(5, 64, T, _cfg(PROB=0.0), device=DEV).any()


def test_drawn_records_statistics():
    for seed, T in ((SEEDS[1], 8), (SEEDS[2], 32), (SEEDS[3], 63)):
        rec = ops.spec_augment_records(seed, 4096, T, device=DEV).cpu().numpy().astype(np.int64)
        assert np.array_equal(rec, ref.draw_records(seed, 4096, T))
        share, counts, _ = ref.statistics(seed, 4096, T)
        assert abs(share - 0.8) <= 0.03                                                     # five binomial standard deviations
        assert (counts > 0).all() and counts.shape == (13,)                                 # every frequency width 0 .. 12 occurs
        assert (rec >= 0).all() and (rec[:, 0:8:2] + rec[:, 1:8:2] <= 80).all() and (rec[:, 8:16:2] + rec[:, 9:16:2] <= T).all()
        assert rec[:, 9:16:2].max() == ref.time_max(0.125, T) and rec[:, 1:8:2].max() == 12


@pytest.mark.parametrize("fill", FILLS, ids=lambda f: str(f))
@pytest.mark.parametrize("T", (8, 32, 63))
def test_seed_form_equals_records_form(T, fill):
    B = 259
    mel = torch.from_numpy(np.array(_case(B, T)[0])).to(DEV).view(B, 1, 80, T)
    cfg = _cfg(FILL=fill)
    for seed in SEEDS[1:3]:
        rec = ops.spec_augment_records(seed, B, T, cfg, device=DEV)
        a, b = ops.spec_augment(mel, seed=seed, config=cfg), ops.spec_augment(mel, rec, config=cfg)
        assert torch.equal(a, b) and not torch.equal(a, mel)
        x = mel.clone()
        ops.spec_augment(x, seed=seed, config=cfg, out=x)
        assert torch.equal(x, a)
        m = ref.masks(rec.cpu().numpy(), T)
        got = a.cpu().numpy().reshape(B, 80, T)
        assert np.array_equal(got.view(np.int32)[~m], _case(B, T)[0].view(np.int32)[~m])
        if fill != "mean":
            assert np.array_equal(got, ref.apply(_case(B, T)[0], rec.cpu().numpy(), fill))


# ---- integration: a dozen synthetic one-second files, batch 5 ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("specaug")
    clips = synth.make_clips(0, 12)
    paths = []
    for i in range(12):
        paths.append(os.path.join(d, f"clip_{i:02d}.wav"))
        synth.write_wav16(paths[-1], clips[i])
    return paths


def _dataset(files, config, augment=True):
    proc = pkg.AudioProcessor(device=DEV)
    proc.set_spec_augment(config)
    return pkg.WakewordDataset(files[:6], files[6:], proc, augment=augment, verbose=False)


def _run(loader, seed=3):
    random.seed(seed)
    torch.manual_seed(seed)
    out = [(d.clone(), t.clone()) for d, t in loader]
    torch.cuda.synchronize()
    return out, random.getstate()


@pytest.mark.parametrize("kind", ("files", "bank"))
def test_loaders_equal_a_hand_written_loop(files, kind):
    ds = _dataset(files, SpecAugmentConfig)
    proc = ds.processor
    loader = ds.loader(5) if kind == "files" else ds.cache().loader(5, augment=True)
    got, state = _run(loader)
    assert [d.shape[0] for d, _ in got] == [5, 5, 2]
    # by hand: same order, augment_batch, mel_batch(normalize=False), spec_augment_batch(inplace=True)
    random.seed(3)
    torch.manual_seed(3)
    masked_any = False
    for k, s in enumerate(range(0, 12, 5)):
        pcm, ok = proc.load_clips_gpu(ds.files[s:s + 5])
        assert ok.all()
        mel = proc.mel_batch(proc.augment_batch(pcm), normalize=False)
        plain = mel.clone()
        assert proc.spec_augment_batch(mel, inplace=True) is mel
        assert torch.equal(got[k][0], mel)
        masked_any |= not torch.equal(plain, mel)
    assert masked_any and random.getstate() == state


@pytest.mark.parametrize("kind", ("files", "bank"))
def test_validation_loaders_are_untouched(files, kind):
    def make(config, augment):
        ds = _dataset(files, config, augment=augment)
        return ds.loader(5) if kind == "files" else ds.cache().loader(5, augment=augment)
    control, control_state = _run(make(None, False))
    got, state = _run(make(SpecAugmentConfig, False))
    assert state == control_state and len(got) == len(control) == 3
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(got, control))
    # and with augment=True the switch costs exactly one 64-bit draw per batch
    aug_control, aug_control_state = _run(make(None, True))
    aug, aug_state = _run(make(SpecAugmentConfig, True))
    assert aug_state != aug_control_state and torch.equal(aug[0][1], aug_control[0][1])


def test_process_audio_file_masks_with_the_seed_it_drew(files):
    ds = _dataset(files, SpecAugmentConfig)
    proc = ds.processor
    hit = False
    for seed in range(4):
        random.seed(seed)
        got = proc.process_audio_file(files[seed], augment=True)
        state = random.getstate()
        assert got.shape == (80, 32) and got.dtype == np.float32
        random.seed(seed)                                           # by hand: the plan, the log-mel, then the masking seed
        pcm, _ = proc.load_clips_gpu([files[seed]])
        plain = proc.mel_batch(proc.augment_batch(pcm), normalize=False)
        drawn = random.getrandbits(64)
        assert random.getstate() == state
        rec = ops.spec_augment_records(drawn, 1, 32, device=DEV).cpu().numpy()
        m = ref.masks(rec, 32)[0]
        want = plain.cpu().numpy().reshape(1, 80, 32)
        assert np.array_equal(got.view(np.int32)[~m], want[0].view(np.int32)[~m])
        if m.any():
            hit = True
            v = got[m]
            exact = ref.fills(want, "mean")[0]
            assert (v == v[0]).all() and abs(float(v[0]) - exact) <= np.spacing(np.float32(abs(exact)))
        item, label = ds[seed]
        assert item.shape == (1, 80, 32) and int(label) == 1
    assert hit
    random.seed(0)
    assert np.array_equal(proc.process_audio_file(files[0], augment=False),
                          pkg.AudioProcessor(device=DEV).process_audio_file(files[0], augment=False))


def test_trainer_steps_on_masked_batches(files):
    ds = _dataset(files, _cfg(PROB=1.0))
    torch.manual_seed(0)
    model = pkg.SimpleWakewordModel().to(DEV)
    trainer = pkg.WakewordTrainer(model, DEV)
    model.train()
    random.seed(5)
    losses = [float(trainer.step(data, target)) for data, target in list(ds.cache().loader(5, augment=True))[:2]]
    assert len(losses) == 2 and all(np.isfinite(losses))
