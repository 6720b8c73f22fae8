"""Inference at clip lengths from 0.25 s to 2 s (AudioConfig.DURATION in [0.25, 2.0]): the any-length log-mel kernels, the column-tiled
conv stack for 33..63 frames and the composed PCM -> logits entry point, against the length-generic CPU oracle.

Tolerances are the 1 s path's: 1e-4 dB on log-mel values, 1e-3 on logits, and for the split-precision conv arithmetic the guard of
tests/test_gpu_guards.py (pooled error <= 2 x the exact-fp32 kernels' + 2^-22).
"""
import os
import random
import struct
import zlib

import numpy as np
import pytest
import torch

import wakeword_jupyterlab_amd as pkg
from oracle import mel_oracle, model_oracle
from wakeword_jupyterlab_amd import ops
from wakeword_jupyterlab_amd.config import AudioConfig, n_frames, n_samples
from wavio import _read_wav

pytestmark = pytest.mark.gpu

MEL_TOL = 1e-4
LOGIT_TOL = 1e-3
POOLED_REL_CAP = 1e-5
SPLIT_EPS = 2.0 ** -22
WIDTHS = [33, 40, 47, 55, 62, 63]


def _cfg(duration):
    return type(f"AudioConfig{duration}", (AudioConfig,), {"DURATION": duration})


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(params=["f16x3", "f32"])
def conv_math(request):
    ops.set_conv_math(request.param)
    yield request.param
    ops.set_conv_math("f16x3")


def _oracle_mel(x, n, normalize):
    """process_audio_file's numeric part at clip length n: normalise -> right zero-pad to n -> log-mel [80, 1 + n // 512]."""
    basis = mel_oracle.mel_filterbank()
    out = []
    for clip in x:
        a = np.asarray(clip, dtype=np.float32)
        if normalize:
            a = mel_oracle.normalize_audio(a).astype(np.float32)
        a = np.pad(a, (0, n - len(a)))
        out.append(mel_oracle.power_to_db_librosa32(mel_oracle.melspectrogram_librosa32(a, basis))[None])
    return np.stack(out).astype(np.float32)


def _tones(n):
    """Noise-free signals: bands 60-80 dB under the peak sit on a float32 FFT's rounding floor (auto mode's case)."""
    t = np.arange(n) / 16000.0
    sig = [np.sin(2 * np.pi * 440 * t), np.sin(2 * np.pi * 3000 * t) + 1e-3 * np.sin(2 * np.pi * 700 * t),
           np.sign(np.sin(2 * np.pi * 150 * t)), np.where((t > 0.1) & (t < 0.2), np.sin(2 * np.pi * 1000 * t), 0.0)]
    imp = np.zeros(n)
    imp[n // 3] = 1.0
    sig.append(imp)
    return np.stack(sig).astype(np.float32)


def _packed(sd, dev):
    return torch.from_numpy(ops.pack_state_dict(sd)).to(dev)


def _model(arch, sd, dev, cfg):
    m = pkg.SimpleWakewordModel(audio_config=cfg) if arch == "simple" else pkg.WakewordModel(audio_config=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).eval()


# ------------------------------------------------------------------------------------------------ K1, any length
@pytest.mark.parametrize("mode", ["auto", "f64", "f32"])
@pytest.mark.parametrize("duration", [0.25, 0.5, 0.75, 1.5, 2.0])
def test_logmel_frames_matches_oracle(dev, duration, mode):
    n = n_samples(_cfg(duration))
    T = n_frames(_cfg(duration))
    full = pkg.synth.make_clips(0, 4, n=n)
    short = pkg.synth.make_clips(10, 3, n=n)[:, : n - 1237].copy()      # rows right-zero-padded to n
    ops.set_logmel_math(mode)
    try:
        res = {}
        for tag, x in (("full", full), ("short", short)):
            for norm in (True, False):
                res[tag, norm] = ops.logmel_frames(torch.from_numpy(x).to(dev), n, norm).cpu().numpy()
        clean = ops.logmel_frames(torch.from_numpy(_tones(n)).to(dev), n, True).cpu().numpy() if mode != "f32" else None
    finally:
        ops.set_logmel_math("auto")
    for (tag, norm), out in res.items():
        x = full if tag == "full" else short
        assert out.shape == (len(x), 1, 80, T)
        ref = _oracle_mel(x, n, norm)
        assert np.abs(out - ref).max() <= MEL_TOL, (tag, norm, np.abs(out - ref).max())
        assert np.all(out.max(axis=(1, 2, 3)) == 0.0) and out.min() >= -80.0
    if clean is not None:                 # noise-free signals: the auto and f64 modes only, as for 1 s clips
        ref = _oracle_mel(_tones(n), n, True)
        assert np.abs(clean - ref).max() <= MEL_TOL, np.abs(clean - ref).max(axis=(1, 2, 3))
        assert np.all(clean.max(axis=(1, 2, 3)) == 0.0) and clean.min() >= -80.0


@pytest.mark.parametrize("mode", ["auto", "f32"])
def test_logmel_frames_large_batch_matches_single_clips(dev, mode):
    """More clips than CUs: the 4-wave form; every clip equals its batch-of-1 result (the 8-wave form) bit for bit.  300 clips are fewer
    than the float kernel's grid of 2 per CU on a 256-CU part, so no float workgroup takes a second clip here (only auto's
    logmel64_kernel<., 64>, 1 per CU, may); the clip loop itself is entered in tests/test_gpu_logmel_carry.py."""
    n = 24000
    x = pkg.synth.make_clips(0, 300, n=n)
    x[::7] = _tones(n)[np.arange(len(x[::7])) % 5]                       # noise-free clips among them: auto mode redoes those
    ops.set_logmel_math(mode)
    try:
        out = ops.logmel_frames(torch.from_numpy(x).to(dev), n, True).cpu().numpy()
        ones = [ops.logmel_frames(torch.from_numpy(x[i:i + 1]).to(dev), n, True).cpu().numpy() for i in (0, 7, 150, 299)]
    finally:
        ops.set_logmel_math("auto")
    for j, i in enumerate((0, 7, 150, 299)):
        assert np.array_equal(ones[j][0], out[i])
    sel = np.arange(0, 300, 13)
    err = np.abs(out[sel] - _oracle_mel(x[sel], n, True)).max(axis=(1, 2, 3))
    noisy = sel % 7 != 0
    assert err[noisy].max() <= MEL_TOL
    if mode == "auto":
        assert err.max() <= MEL_TOL


def test_logmel_frames_at_one_second_is_the_existing_kernel(dev):
    x = torch.from_numpy(pkg.synth.make_clips(0, 9)).to(dev)
    for norm in (True, False):
        assert torch.equal(ops.logmel_frames(x, 16000, norm), ops.logmel(x, norm))
        assert torch.equal(ops.logmel_frames(x[:, :12345], 16000, norm), ops.logmel(x[:, :12345], norm))


# ------------------------------------------------------------------------------------------------ K2, 33..63 columns
def _seam_columns(width, arch):
    """The columns on both sides of every tile edge and every owned-range boundary of the column tiling (csrc/ww_cnn.hip, ColTiling)."""
    h = 3 if arch == "full" else 2
    step = 32 - 2 * h
    K = 1 + -(-(width - 32) // step)
    cols = set()
    for k in range(K):
        s = width - 32 if k == K - 1 else k * step
        lo = 0 if k == 0 else k * step + h
        for c in (s, s + 1, s + h - 1, s + h, lo - 1, lo, lo + 1, s + 31 - h, s + 32 - h, s + 30, s + 31):
            if 0 <= c < width:
                cols.add(c)
    return sorted(cols)


def _seam_input(width, batch, arch, seed):
    """Log-mel-like images with impulses and large values in the columns on both sides of every tile seam."""
    r = np.random.default_rng(seed)
    x = (r.standard_normal((batch, 1, 80, width)) * 15 - 35).clip(-80, 0).astype(np.float32)
    cols = _seam_columns(width, arch)
    for i in range(batch):
        c = cols[i % len(cols)]
        x[i, 0, r.integers(80), c] = 40.0                                   # an impulse
        x[i, 0, :, cols[(i + 3) % len(cols)]] += 25.0                     # a whole large column
    return x


def _pooled_rel(got, ref):
    scale = np.abs(ref).max(axis=1, keepdims=True)
    scale[scale == 0] = 1.0
    return float((np.abs(got.astype(np.float64) - ref) / scale).max())


@pytest.mark.parametrize("arch", ["simple", "full"])
@pytest.mark.parametrize("width", WIDTHS)
def test_wide_conv_stack_matches_oracle(dev, conv_math, arch, width):
    sd = pkg.synth.make_state_dict(arch, seed=1234)
    n_conv = 2 if arch == "simple" else 3
    x = _seam_input(width, 5, arch, width)
    packed = _packed(sd, dev)
    pooled = ops.cnn_pool_wide(torch.from_numpy(x).to(dev), packed, n_conv).cpu().numpy()
    ref_pooled = model_oracle.pooled_features_np(x, sd)
    assert _pooled_rel(pooled, ref_pooled) <= POOLED_REL_CAP
    cfg = _cfg(2.0)
    with torch.no_grad():
        y = _model(arch, sd, dev, cfg)(torch.from_numpy(x).to(dev)).cpu().numpy()
    assert np.abs(y - model_oracle.forward_np(x, sd)).max() <= LOGIT_TOL


@pytest.mark.parametrize("arch", ["simple", "full"])
@pytest.mark.parametrize("batch", [1, 5, 300])
def test_wide_conv_stack_odd_batches(dev, conv_math, arch, batch):
    sd = pkg.synth.make_state_dict(arch, seed=7)
    n_conv = 2 if arch == "simple" else 3
    x = _seam_input(47, batch, arch, batch)
    got = ops.cnn_pool_wide(torch.from_numpy(x).to(dev), _packed(sd, dev), n_conv).cpu().numpy()
    sel = np.unique(np.r_[0, batch // 2, batch - 1])
    assert _pooled_rel(got[sel], model_oracle.pooled_features_np(x[sel], sd)) <= POOLED_REL_CAP


def _adversarial(arch, case):
    sd = {k: v.copy() for k, v in pkg.synth.make_state_dict(arch, seed=21).items()}
    r = np.random.default_rng(zlib.crc32(case.encode()) % 1000)
    keys = [k for k in sd if k.startswith("conv") and k.endswith("weight")] + ["lstm.weight_ih_l0", "lstm.weight_ih_l1"]
    if case == "lognormal":
        for k in keys:
            sd[k] = (sd[k] * np.exp(2.0 * r.standard_normal(sd[k].shape))).astype(np.float32)
    elif case == "outlier_x1000":
        for k in keys:
            flat = sd[k].reshape(-1)
            flat[int(r.integers(flat.size))] *= 1000.0
    return sd


@pytest.mark.parametrize("arch", ["simple", "full"])
@pytest.mark.parametrize("width", [47, 63])
@pytest.mark.parametrize("case", ["lognormal", "outlier_x1000", "one_hot_1e6_at_seams", "mixed_per_clip"])
def test_split_precision_guard_on_wide_images(dev, arch, width, case):
    """At T = 47 and 63 the f16x3 kernels' pooled error against float64 stays within 2 x the exact-fp32 kernels' + 2^-22, as
    tests/test_gpu_guards.py demands at T = 32 and with its construction: adversarial weights on log-mel-range inputs, adversarial
    inputs (a huge pixel in the columns around the tile seams, a per-clip magnitude spread) on ordinary weights."""
    r = np.random.default_rng(width)
    x = _seam_input(width, 6, arch, width)
    if case in ("lognormal", "outlier_x1000"):
        sd = _adversarial(arch, case)
    else:
        sd = {k: v.copy() for k, v in pkg.synth.make_state_dict(arch, seed=21).items()}
        x = (r.standard_normal((6, 1, 80, width)) * 1e-2).astype(np.float32)
        if case == "one_hot_1e6_at_seams":           # one huge pixel per clip, next to a seam of every tile in turn
            cols = _seam_columns(width, arch)
            for i in range(6):
                x[i, 0, 40, cols[(i * len(cols)) // 6]] = 1e6
        else:
            x = (x * 100 * (10.0 ** np.arange(-4, 8, 2))[:, None, None, None]).astype(np.float32)
    n_conv = 2 if arch == "simple" else 3
    ref = model_oracle.pooled_features_np(x, sd)
    packed = _packed(sd, dev)
    errs = {}
    try:
        for mode in ("f32", "f16x3"):
            ops.set_conv_math(mode)
            got = ops.cnn_pool_wide(torch.from_numpy(x).to(dev), packed, n_conv).cpu().numpy()
            assert np.isfinite(got).all()
            errs[mode] = _pooled_rel(got, ref)
    finally:
        ops.set_conv_math("f16x3")
    assert errs["f32"] <= POOLED_REL_CAP and errs["f16x3"] <= 2 * errs["f32"] + SPLIT_EPS, errs


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("arch", ["simple", "full"])
def test_wide_results_do_not_depend_on_the_batch(dev, conv_math, arch):
    sd = pkg.synth.make_state_dict(arch, seed=3)
    n_conv = 2 if arch == "simple" else 3
    n = 32000
    pcm = torch.from_numpy(pkg.synth.make_clips_tiled(0, 4096, unique=64, n=n)).to(dev)
    packed = _packed(sd, dev)
    big = ops.forward_pcm_frames(pcm, packed, n_conv, n)
    again = ops.forward_pcm_frames(pcm, packed, n_conv, n)
    assert torch.equal(big, again)
    for i in (0, 1, 2049, 4095):
        assert torch.equal(ops.forward_pcm_frames(pcm[i:i + 1], packed, n_conv, n), big[i:i + 1])
    mel = ops.logmel_frames(pcm[:8], n, True)
    assert torch.equal(ops.lstm_fc(ops.cnn_pool_wide(mel, packed, n_conv), packed, n_conv), big[:8])


@pytest.mark.parametrize("arch", ["simple", "full"])
def test_one_second_through_the_new_entry_points_is_bit_identical(dev, conv_math, arch):
    sd = pkg.synth.make_state_dict(arch, seed=1234)
    n_conv = 2 if arch == "simple" else 3
    packed = _packed(sd, dev)
    pcm = torch.from_numpy(pkg.synth.make_clips(0, 37)).to(dev)
    assert torch.equal(ops.forward_pcm_frames(pcm, packed, n_conv, 16000), ops.forward_pcm(pcm, packed, n_conv))
    mel = ops.logmel(pcm, True)
    assert torch.equal(ops.cnn_pool_wide(mel, packed, n_conv), ops.cnn_pool(mel, packed, n_conv))
    assert torch.equal(ops.cnn_pool_wide(mel[..., :20].contiguous(), packed, n_conv), ops.cnn_pool(mel[..., :20].contiguous(), packed, n_conv))
    with torch.no_grad():
        assert torch.equal(_model(arch, sd, dev, AudioConfig).forward_pcm(pcm), ops.forward_pcm(pcm, packed, n_conv))


# ------------------------------------------------------------------------------------------------ models at 1.5 s / 2 s
@pytest.mark.parametrize("arch", ["simple", "full"])
@pytest.mark.parametrize("duration", [0.25, 1.5, 2.0])
def test_models_at_other_durations_match_the_oracle_chain(dev, arch, duration):
    cfg = _cfg(duration)
    n, T = n_samples(cfg), n_frames(cfg)
    sd = pkg.synth.make_state_dict(arch, seed=1234)
    m = _model(arch, sd, dev, cfg)
    x = pkg.synth.make_clips(20, 6, n=n)
    x[5, n // 2:] = 0.0
    short = x[:, : n - 999].copy()
    ref_mel = _oracle_mel(x, n, True)
    proc = pkg.AudioProcessor(cfg)
    with torch.no_grad():
        mel = proc.mel_batch(x)
        y_mel = m(mel).cpu().numpy()
        y_pcm = m.forward_pcm(torch.from_numpy(x).to(dev)).cpu().numpy()
        y_short = m.forward_pcm(torch.from_numpy(short).to(dev)).cpu().numpy()
    assert mel.shape == (6, 1, 80, T) and np.abs(mel.cpu().numpy() - ref_mel).max() <= MEL_TOL
    assert proc.audio_to_mel(x[0] / np.abs(x[0]).max()).shape == (80, T)
    ref = model_oracle.forward_np(ref_mel, sd)
    assert np.abs(y_mel - ref).max() <= LOGIT_TOL and np.abs(y_pcm - ref).max() <= LOGIT_TOL
    assert np.abs(y_short - model_oracle.forward_np(_oracle_mel(short, n, True), sd)).max() <= LOGIT_TOL
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 1, 80, max(32, T) + 1, device=dev))


def test_default_model_still_refuses_33_frames_and_training_refuses_wide_images(dev):
    m = pkg.SimpleWakewordModel().to(dev).eval()
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 1, 80, 33, device=dev))
    m15 = pkg.WakewordModel(audio_config=_cfg(1.5)).to(dev).train()
    with pytest.raises(NotImplementedError):
        m15(torch.zeros(2, 1, 80, 47, device=dev))


def test_direct_f16_arithmetic_refuses_wide_images_instead_of_switching_forms(dev):
    sd = pkg.synth.make_state_dict("simple", seed=1)
    packed = _packed(sd, dev)
    ops.set_conv_math("f16x3d")
    try:
        x = torch.zeros(2, 1, 80, 47, device=dev)
        with pytest.raises(RuntimeError, match="DIRECT"):
            ops.cnn_pool_wide(x, packed, 2)
        ops.cnn_pool_wide(x[..., :32].contiguous(), packed, 2)          # the 1 s kernels still run it up to 32 columns
    finally:
        ops.set_conv_math("f16x3")


# ------------------------------------------------------------------------------------------------ files -> logits at 1.5 s
def _write_wav16(path, x, sr=16000):
    raw = np.clip(np.round(np.asarray(x, np.float64) * 32767), -32768, 32767).astype("<i2").tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, sr, sr * 2, 2, 16)
                + b"data" + struct.pack("<I", len(raw)) + raw)


def _oracle_file_mel(path, n, rng):
    """load (16 kHz PCM-16) -> normalize_audio over the whole file -> pad_or_truncate(n) with the seeded crop -> log-mel [80, T]."""
    a, _ = _read_wav(path)
    a = mel_oracle.normalize_audio(a[:, 0].astype(np.float32)).astype(np.float32)
    a = mel_oracle.pad_or_truncate(a, n, rng)
    return mel_oracle.power_to_db_librosa32(mel_oracle.melspectrogram_librosa32(a.astype(np.float32), mel_oracle.mel_filterbank()))


@pytest.mark.parametrize("arch", ["simple", "full"])
def test_wav_files_through_dataset_loader_and_model_at_1_5_s(dev, tmp_path, arch):
    """1.5 s and 3 s WAV files -> AudioProcessor(DURATION 1.5) -> WakewordDataset(augment=False) -> DataLoader -> WakewordModel(audio_config)
    .eval(): K0 crops / pads to 24,000 samples with python `random`'s draws (seeded), K1 gives [B,1,80,47], and the result matches the
    decode + mel + model oracle chain; an unreadable file is a zero item of width 47."""
    cfg = _cfg(1.5)
    n, T = n_samples(cfg), n_frames(cfg)
    lens = [24000, 48000, 30001, 11000, 48000, 24000]
    wake, neg = [], []
    for i, ln in enumerate(lens):
        p = os.path.join(tmp_path, f"f{i}.wav")
        _write_wav16(p, pkg.synth.make_clip(i, ln) * 0.4)
        (wake if i % 2 == 0 else neg).append(p)
    bad = os.path.join(tmp_path, "bad.wav")
    with open(bad, "wb") as f:
        f.write(b"not a wav file")
    neg.append(bad)
    proc = pkg.AudioProcessor(cfg)
    ds = pkg.WakewordDataset(wake, neg, proc, augment=False, verbose=False)
    sd = pkg.synth.make_state_dict(arch, seed=1234)
    model = _model(arch, sd, dev, cfg)
    random.seed(11)
    datas, targets = [], []
    with torch.no_grad():
        for data, target in pkg.DataLoader(ds, batch_size=4, shuffle=False):
            assert data.shape[1:] == (1, 80, T)
            datas.append(data)
            targets.append(target)
    data = torch.cat(datas)
    rng = random.Random(11)
    ref = []
    for p in ds.files:
        ref.append(np.zeros((80, T), np.float32) if p == bad else _oracle_file_mel(p, n, rng))
    ref = np.stack(ref)[:, None]
    got = data.cpu().numpy()
    assert np.abs(got - ref).max() <= MEL_TOL
    with torch.no_grad():
        y = model(data).cpu().numpy()
    assert np.abs(y - model_oracle.forward_np(ref, sd)).max() <= LOGIT_TOL
    assert torch.equal(torch.cat(targets).cpu().view(-1), torch.tensor(ds.labels))
    # the per-item path and predict_wakeword at the model's duration, with the same seeded crops
    random.seed(5)
    item, _ = ds[1]                                         # a 3 s file: cropped to 1.5 s
    mel_ref = _oracle_file_mel(ds.files[1], n, random.Random(5))
    assert item.shape == (1, 80, T) and np.abs(item[0].numpy() - mel_ref).max() <= MEL_TOL
    random.seed(5)
    is_wake, prob = pkg.predict_wakeword(ds.files[1], model, proc, dev, threshold=0.5)
    logits = model_oracle.forward_np(mel_ref[None, None], sd)[0]
    p_ref = float(np.exp(logits[1]) / np.exp(logits).sum())
    assert abs(prob - p_ref) <= 1e-3 and is_wake == (prob >= 0.5)
    bad_item, _ = ds[len(ds.files) - 1]
    assert bad_item.shape == (1, 80, T) and not bad_item.any()
