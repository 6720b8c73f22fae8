"""Background noise at a random SNR on the GPU: the mix kernel against a float64 numpy restatement of its definition (written here), its
composition with the rest of KA, the graph-capturable records path, the device-resident bank built from WAV and FLAC files, a bank of more
than 2^31 samples, and the training flow with a bank attached.

Definition ("Background noise"): seg[j] = bank[off + (start + j) mod len]; Ex = sum x^2, En = sum seg^2;
g = sqrt(Ex / (En 10^(snr/10))); out = fma(g, seg, x) in float32 -- nothing added when Ex or En is 0.  Tolerance per sample:
2^-22 max(|x|, |g seg|) (the float32 gain and the fma's rounding), and the SNR measured on the output within 1e-4 dB of the drawn one."""
import copy
import ctypes as C
import random

import numpy as np
import pytest
import torch

import flacenc
import wakeword_jupyterlab_amd as pkg
from oracle import augment_oracle as ao
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import ops
from wakeword_jupyterlab_amd.audio import AudioProcessor
from wakeword_jupyterlab_amd.background import BackgroundNoiseBank
from wakeword_jupyterlab_amd.config import AudioConfig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OFF = {"shift": 0, "n_steps": None, "rate": None, "crop": 0, "sigma": 0.0, "seed": 0}
NS = (4000, 5001, 12345, 16000, 16383)
SNRS = (-5.0, 0.0, 20.0, 40.0)


def _cfg(duration):
    return type("Cfg", (AudioConfig,), {"DURATION": duration})


def _clips(count, n, start=0):
    x = pkg.synth.make_clips(start, count, n=n)
    return np.ascontiguousarray(x / np.abs(x).max(axis=1, keepdims=True), dtype=np.float32)


def _noise_files(lengths, seed=0):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * (0.05 + 0.3 * i)).astype(np.float32) for i, n in enumerate(lengths)]


def _bank(files):
    data = torch.from_numpy(np.concatenate(files)).to(DEV)
    return BackgroundNoiseBank.from_buffer(data, [len(f) for f in files])


def _want(x, f, start, snr):
    """The definition in float64: (out, g * seg)."""
    n = len(x)
    seg = f[(start + np.arange(n)) % len(f)].astype(np.float64)
    x64 = x.astype(np.float64)
    ex, en = (x64 ** 2).sum(), (seg ** 2).sum()
    if ex == 0 or en == 0:
        return x64, np.zeros(n)
    g = np.sqrt(ex / (en * 10.0 ** (snr / 10.0)))
    return x64 + g * seg, g * seg


def _check_mix(got, x, f, start, snr):
    want, gs = _want(x, f, start, snr)
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= 2.0 ** -22 * np.maximum(np.abs(x), np.abs(gs))).all(), float((err / np.maximum(np.abs(x), np.abs(gs))).max())
    added = got.astype(np.float64) - x.astype(np.float64)
    measured = 10 * np.log10((x.astype(np.float64) ** 2).sum() / (added ** 2).sum())
    assert abs(measured - snr) <= 1e-4, (measured, snr)


def _bg_plans(files_, starts, snrs, base=None):
    return [dict(base or OFF, bg_file=f, bg_start=s, snr_db=r) for f, s, r in zip(files_, starts, snrs)]


@pytest.mark.parametrize("n", NS)
def test_mix_matches_the_definition(n):
    """Standalone and fused forms, every SNR, starts that wrap, and a file shorter than the clip (it repeats)."""
    files = _noise_files([3 * n + 17, 777, n + 1], seed=n)
    bank = _bank(files)
    cases = [(f, s, r) for r in SNRS for f, s in ((0, 0), (0, 3 * n + 16), (1, 776), (1, 5), (2, n // 2))]
    B = len(cases)
    x = _clips(B, n, start=n % 97)
    xt = torch.from_numpy(x).to(DEV)
    fs, ss, rs = zip(*cases)
    mixed = ops.mix_background(xt, bank, fs, ss, rs).cpu().numpy()
    fused = ops.augment(xt, _bg_plans(fs, ss, rs), bank=bank).cpu().numpy()
    for i, (f, s, r) in enumerate(cases):
        _check_mix(mixed[i], x[i], files[f], s, r)
    assert np.array_equal(fused.view(np.uint32), mixed.view(np.uint32))


def test_standalone_mix_takes_every_inference_length():
    files = _noise_files([40000, 900], seed=3)
    bank = _bank(files)
    for n in (4000, 16384, 16385, 24000, 32000):
        x = _clips(4, n, start=n % 13)
        got = ops.mix_background(torch.from_numpy(x).to(DEV), bank, [0, 1, 0, 1], [39999, 0, 123, 899], [3.0, 10.0, -5.0, 40.0]).cpu().numpy()
        for i, (f, s, r) in enumerate(zip([0, 1, 0, 1], [39999, 0, 123, 899], [3.0, 10.0, -5.0, 40.0])):
            _check_mix(got[i], x[i], files[f], s, r)
    with pytest.raises(ValueError):
        ops.mix_background(torch.zeros(2, 32001, device=DEV), bank, 0, 0, 10.0)


@pytest.mark.parametrize("n", (16000, 8000))
def test_fused_without_gaussian_noise_is_augment_then_mix(n):
    """roll / pitch / stretch + background with sigma 0 == augment without background, then mix_background: bit for bit."""
    B = 24
    x = torch.from_numpy(_clips(B, n, start=5)).to(DEV)
    files = _noise_files([20000, 3000, 650], seed=7)
    bank = _bank(files)
    rng = random.Random(n)
    base = [dict(ao.draw_plan(rng, n=n), sigma=0.0, seed=0) for _ in range(B)]
    fs = [rng.randrange(3) for _ in range(B)]
    ss = [rng.randrange(len(files[f])) for f in fs]
    rs = [rng.uniform(-5, 40) for _ in range(B)]
    plans = [dict(p, bg_file=f, bg_start=s, snr_db=r) for p, f, s, r in zip(base, fs, ss, rs)]
    fused = ops.augment(x, plans, bank=bank)
    two = ops.mix_background(ops.augment(x, base), bank, fs, ss, rs)
    assert torch.equal(fused, two)


@pytest.mark.parametrize("n", (16000, 12345))
def test_clips_without_background_keep_their_bits(n):
    """With a bank: clips whose plan has no background give ops.augment's bits (Gaussian noise on), inside a batch that mixes and in a batch
    where nobody does; a clip with background and noise is the mix plus the same noise."""
    B = 16
    x = torch.from_numpy(_clips(B, n, start=30)).to(DEV)
    bank = _bank(_noise_files([25000, 1200], seed=11))
    rng = random.Random(3)
    base = [ao.draw_plan(rng, n=n) for _ in range(B)]
    for p in base:
        p["sigma"], p["seed"] = 0.15, rng.getrandbits(32)
    plain = ops.augment(x, base)
    plans = [dict(p, bg_file=i % 2, bg_start=rng.randrange(1200), snr_db=10.0) if i % 3 == 0 else dict(p) for i, p in enumerate(base)]
    got = ops.augment(x, plans, bank=bank)
    for i in range(B):
        if i % 3:
            assert torch.equal(got[i], plain[i])
        else:
            assert not torch.equal(got[i], plain[i])
    assert torch.equal(ops.augment(x, [dict(p) for p in base], bank=bank), plain)
    # noise after the mix: (fused with noise) - (fused without noise) is the noise alone, as in the plain clips
    quiet = ops.augment(x, [dict(p, sigma=0.0) for p in plans], bank=bank)
    quiet_plain = ops.augment(x, [dict(p, sigma=0.0) for p in base])
    d_bg = (got - quiet)[0].double()
    d_plain = (plain - quiet_plain)[0].double()
    assert torch.allclose(d_bg, d_plain, atol=4e-6)


def test_batch_independent_and_repeatable():
    n, B = 16000, 20
    x = torch.from_numpy(_clips(B, n, start=70)).to(DEV)
    bank = _bank(_noise_files([40000, 500, 16001], seed=2))
    rng = random.Random(9)
    plans = [dict(ao.draw_plan(rng), bg_file=i % 3, bg_start=rng.randrange(500), snr_db=rng.uniform(0, 40)) for i in range(B)]
    a = ops.augment(x, plans, bank=bank)
    b = ops.augment(x, plans, bank=bank)
    assert torch.equal(a, b)
    perm = list(range(B))[::-1]
    c = ops.augment(x[perm].contiguous(), [plans[i] for i in perm], bank=bank)
    assert torch.equal(c, a[perm])
    for i in (0, 7, 19):
        assert torch.equal(ops.augment(x[i:i + 1].contiguous(), [plans[i]], bank=bank)[0], a[i])


def _arrays(plans, bank):
    arr = (nat.AugmentPlan * len(plans))()
    bg = (nat.AugmentBg * len(plans))()
    for a, b, p in zip(arr, bg, plans):
        a.shift, a.crop_start = p["shift"], p["crop"]
        a.pitch_rate = ao.pitch_rate(p["n_steps"]) if p["n_steps"] is not None else 0.0
        a.stretch_rate = p["rate"] or 0.0
        a.noise_sigma, a.noise_seed = p["sigma"], p["seed"]
        if "bg_file" in p:
            f = p["bg_file"]
            b.file_offset, b.file_len, b.start, b.snr_db, b.enabled = int(bank.offsets[f]), int(bank.lengths[f]), p["bg_start"], p["snr_db"], 1
    return arr, bg


@pytest.mark.parametrize("n", (16000, 8000))
def test_records_path_is_graph_capturable_and_bitwise_equal(n):
    """ww_augment_bg_prepare + ww_augment_bg_records_f32, captured once with the records copy and replayed with new records: every replay
    equals the direct call (ops.augment with the bank), a batch without any background included."""
    B = 10
    x = torch.from_numpy(_clips(B, n, start=40)).to(DEV)
    bank = _bank(_noise_files([30000, 2000, 900], seed=4))
    rb = int(nat.lib.ww_augment_bg_record_bytes())
    rec_host = torch.empty(B * rb, dtype=torch.uint8).pin_memory()
    rec_dev = torch.empty(B * rb, dtype=torch.uint8, device=DEV)
    out = torch.empty_like(x)
    ws = torch.empty(int(nat.lib.ww_augment_bg_workspace_bytes(B, n)), dtype=torch.uint8, device=DEV)
    rng = random.Random(78)

    def draw(p_bg):
        plans = []
        for _ in range(B):
            p = ao.draw_plan(rng, n=n)
            if rng.random() < p_bg:
                f = rng.randrange(3)
                p.update(bg_file=f, bg_start=rng.randrange(int(bank.lengths[f])), snr_db=rng.uniform(-5, 40))
            plans.append(p)
        return plans
    batches = [draw(0.8), draw(1.0), draw(0.5), draw(0.0)]

    def prepare(plans):
        arr, bg = _arrays(plans, bank)
        nat.check(nat.lib.ww_augment_bg_prepare(C.cast(arr, C.c_void_p), C.cast(bg, C.c_void_p), B, n, bank.data.numel(),
                                                C.c_void_p(rec_host.data_ptr())))

    def launch(stream):
        nat.check(nat.lib.ww_augment_bg_records_f32(x.data_ptr(), B, n, n, rec_dev.data_ptr(), bank.data.data_ptr(), bank.data.numel(),
                                                    out.data_ptr(), n, ws.data_ptr(), C.c_void_p(stream.cuda_stream)))
    ops.init()
    prepare(batches[0])
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                      # warm-up outside capture (LDS opt-in, tables)
        rec_dev.copy_(rec_host, non_blocking=True)
        launch(side)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        rec_dev.copy_(rec_host, non_blocking=True)
        launch(torch.cuda.current_stream())
    for plans in batches:
        prepare(plans)
        g.replay()
        torch.cuda.synchronize()
        want = ops.augment(x, plans, bank=bank)
        assert torch.equal(out, want)
    assert torch.equal(out, ops.augment(x, batches[-1]))                             # no background: ops.augment's bits


def test_silence_and_silent_noise_leave_the_clip_unchanged():
    n = 16000
    files = [np.zeros(5000, np.float32), _noise_files([7000], seed=1)[0]]
    bank = _bank(files)
    x = _clips(2, n, start=3)
    x[1] = 0.0                                                                        # Ex = 0
    xt = torch.from_numpy(x).to(DEV)
    got = ops.mix_background(xt, bank, [0, 1], [10, 10], [0.0, 0.0])                # En = 0, Ex = 0
    assert torch.equal(got, xt)
    fused = ops.augment(xt, _bg_plans([0, 1], [10, 10], [-5.0, -5.0]), bank=bank)
    assert torch.equal(fused, xt)


def test_bank_from_wav_and_flac_files_equals_load_audio(tmp_path):
    """44.1 kHz stereo WAV, 48 kHz mono WAV, 44.1 kHz stereo FLAC, 48 kHz mono FLAC, a 16 kHz file shorter than a clip and one unreadable
    file: every file's samples equal AudioProcessor.load_audio bit for bit; skipped == 1; the private reader is closed."""
    specs = [("a.wav", 44100, 2, 3 * 44100 + 17), ("b.wav", 48000, 1, 2 * 48000 + 5), ("c.flac", 44100, 2, 44100 + 999),
             ("d.flac", 48000, 1, 3 * 48000), ("e.wav", 16000, 1, 5000)]
    paths = []
    for k, (name, rate, ch, frames) in enumerate(specs):
        x = flacenc.signal(frames, ch, 16, seed=50 + k)
        data = flacenc.encode(x, rate, 16, stereo="independent") if name.endswith(".flac") else flacenc.wav_bytes(x, rate, 16)
        p = tmp_path / name
        p.write_bytes(data)
        paths.append(str(p))
    bad = tmp_path / "broken.wav"
    bad.write_bytes(b"RIFF\x00\x00\x00\x00WAVEjunk")
    paths.insert(2, str(bad))
    bank = BackgroundNoiseBank(paths, device=DEV)
    assert bank.skipped == 1 and bank.n_files == 5
    assert bank.offsets.dtype == np.int64 and bank.lengths.dtype == np.int64
    proc = AudioProcessor()
    good = [p for p in paths if p != str(bad)]
    for i, p in enumerate(good):
        want = proc.load_audio(p)
        got = bank.file(i).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), p
    assert bank.lengths[4] == 5000 < 16000
    st = bank.stats
    assert st["files"] == 5 and st["skipped"] == 1 and st["audio_seconds_per_second"] > 0 and st["files_per_second"] > 0
    # a directory, the cap in list order, and nothing readable
    capped = BackgroundNoiseBank(str(tmp_path), device=DEV, max_seconds=1.0)
    assert capped.n_files == 1 and capped.skipped == 0 and capped.n_samples == bank.lengths[0]      # a.wav alone passes 1 s
    with pytest.raises(ValueError):
        BackgroundNoiseBank([str(bad)], device=DEV)
    # attached to a processor: the drawn segment is mixed into a clip whose length is shorter than e.wav's repeat
    proc.set_background_noise(bank)
    assert proc.background_noise is bank
    random.seed(4)
    z = proc.augment_audio(_clips(1, 16000)[0])
    assert z.shape == (16000,) and np.isfinite(z).all()
    proc.set_background_noise(None)
    assert proc.background_noise is None


def test_bank_past_two_to_the_31_samples():
    """A bank of just over 2^31 samples: a segment near its end (a file that starts past 2^31, wrapping) and one of the first file that
    wraps from its end (past 2^31) to its start mix correctly.  The 8.6 GB are freed after the test."""
    n = 16000
    tail = 60000
    total = 2 ** 31 + tail
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < 4 * total + (2 << 30):
        pytest.fail(f"a bank of {total} samples needs {4 * total / 2**30:.1f} GiB; {free / 2**30:.1f} GiB free")
    data = torch.zeros(total, dtype=torch.float32, device=DEV)
    try:
        f0_len, f1_len = 2 ** 31 + 20000, tail - 20000
        rng = np.random.default_rng(31)
        head0 = (rng.standard_normal(30000) * 0.2).astype(np.float32)          # file 0: its first and last samples are set
        end0 = (rng.standard_normal(9000) * 0.1).astype(np.float32)
        f1 = (rng.standard_normal(f1_len) * 0.3).astype(np.float32)
        data[:30000] = torch.from_numpy(head0).to(DEV)
        data[f0_len - 9000:f0_len] = torch.from_numpy(end0).to(DEV)
        data[f0_len:] = torch.from_numpy(f1).to(DEV)
        bank = BackgroundNoiseBank.from_buffer(data, [f0_len, f1_len])
        assert bank.offsets[1] == f0_len > 2 ** 31
        x = _clips(2, n, start=77)
        xt = torch.from_numpy(x).to(DEV)
        s1, s0 = f1_len - 123, f0_len - 9000
        got = ops.mix_background(xt, bank, [1, 0], [s1, s0], [7.5, 15.0]).cpu().numpy()
        _check_mix(got[0], x[0], f1, s1, 7.5)
        seg0 = np.concatenate([end0, head0])                                   # the last 9000 samples of file 0, then its start
        _check_mix(got[1], x[1], seg0, 0, 15.0)
        fused = ops.augment(xt, _bg_plans([1, 0], [s1, s0], [7.5, 15.0]), bank=bank).cpu().numpy()
        assert np.array_equal(fused.view(np.uint32), got.view(np.uint32))
    finally:
        del data
        bank = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _write_set(tmp_path, n_files, n, start):
    clips = pkg.synth.make_clips(start, n_files, n=n) * 0.8
    paths = []
    for i in range(n_files):
        p = str(tmp_path / f"c{start + i:04d}.wav")
        pkg.synth.write_wav16(p, clips[i])
        paths.append(p)
    return paths


@pytest.mark.parametrize("duration", (1.0, 0.5))
def test_training_flow_with_a_bank(tmp_path, duration):
    """WAV files -> WakewordDataset(augment=True).loader() with a noise directory attached -> one epoch -> a training step; the epoch
    draws background for most clips and repeats bit for bit under the same seeds; the per-item path uses the bank too."""
    cfg = _cfg(duration)
    n = int(16000 * duration)
    paths = _write_set(tmp_path, 10, n, start=500)
    noise_dir = tmp_path / "background_noise"
    noise_dir.mkdir()
    for i, f in enumerate(_noise_files([40000, 6000], seed=8)):
        pkg.synth.write_wav16(str(noise_dir / f"noise_{i}.wav"), f)
    proc = AudioProcessor(cfg)
    bank = proc.set_background_noise(str(noise_dir))
    assert bank.n_files == 2
    ds = pkg.WakewordDataset(paths[:4], paths[4:], proc, augment=True, verbose=False)
    T = 1 + n // 512
    data, _ = ds[0]
    assert data.shape == (1, 80, T) and torch.isfinite(data).all()
    seen = []
    orig = ops.augment

    def spy(pcm, plans, bank=None):
        seen.append((sum("bg_file" in p for p in plans), bank))
        return orig(pcm, plans, bank=bank)
    torch.manual_seed(0)
    model0 = pkg.SimpleWakewordModel(audio_config=cfg).to(DEV)

    def epoch(seed):
        random.seed(seed)
        torch.manual_seed(seed)
        model = copy.deepcopy(model0)
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        crit = torch.nn.CrossEntropyLoss()
        batches = []
        for data, target in ds.loader(batch_size=4, shuffle=True):
            assert data.shape[1:] == (1, 80, T) and torch.isfinite(data).all()
            batches.append(data.clone())
        # the training step that follows
        opt.zero_grad()
        loss = crit(model(batches[0]), torch.tensor([1, 0, 1, 0], device=DEV))
        loss.backward()
        opt.step()
        assert torch.isfinite(loss)
        return batches, [p.detach().clone() for p in model.parameters()]
    ops.augment = spy
    try:
        b1, p1 = epoch(5)
    finally:
        ops.augment = orig
    assert len(b1) == 3 and sum(k for k, _ in seen) >= 4 and all(bk is bank for _, bk in seen)
    assert any(not torch.equal(a, b) for a, b in zip(p1, model0.parameters()))
    b2, p2 = epoch(5)
    assert all(torch.equal(a, b) for a, b in zip(b1, b2)) and all(torch.equal(a, b) for a, b in zip(p1, p2))
    # without the bank the same seed draws the same reference plans but mixes nothing: other batches
    proc.set_background_noise(None)
    b3, _ = epoch(5)
    assert any(not torch.equal(a, b) for a, b in zip(b1, b3))
