"""Reverberation on the GPU: the FFT convolution against the float64 reference of tests/reverb_ref.py, its place in KA, bit identity
with reverb off, independence from the batch, the graph-capturable records path, the bank built from WAV and FLAC files, and a training
epoch with RIR and background banks.

Tolerance: max |out - ref| <= TOL * max |ref| per clip (float32 FFTs of 2^15 points: the worst error measured on the MI355X over the lengths and RIRs below is 3.3e-7)."""
import copy
import ctypes as C
import random
import struct

import numpy as np
import pytest
import torch

import flacenc
import reverb_ref
import wakeword_jupyterlab_amd as pkg
from oracle import augment_oracle as ao
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import ops
from wakeword_jupyterlab_amd.audio import AudioProcessor
from wakeword_jupyterlab_amd.background import BackgroundNoiseBank
from wakeword_jupyterlab_amd.config import AudioConfig
from wakeword_jupyterlab_amd.reverb import ImpulseResponseBank

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TOL = 1e-6
OFF = {"shift": 0, "n_steps": None, "rate": None, "crop": 0, "sigma": 0.0, "seed": 0}
NS = (4000, 8000, 12345, 16000, 16383)
RIR_SPECS = ((1, 0), (97, 10), (4000, 100), (16384, 300), (30000, 500))       # (length, pre-delay); 30000 is cut to 16384 taps


def _clips(count, n, start=0):
    x = pkg.synth.make_clips(start, count, n=n)
    return np.ascontiguousarray(x / np.abs(x).max(axis=1, keepdims=True), dtype=np.float32)


def _rirs():
    return [reverb_ref.decaying_rir(L, d, seed=L, rt_samples=min(3000.0, L / 3 + 1)) for L, d in RIR_SPECS]


def _check(got, x, h):
    kept, dpos = reverb_ref.trim(h)
    want = reverb_ref.reverb(x, kept, dpos)
    err = float(np.abs(got.astype(np.float64) - want).max())
    assert err <= TOL * float(np.abs(want).max()), (err, float(np.abs(want).max()))
    return err / float(np.abs(want).max())


@pytest.fixture(scope="module")
def bank():
    return ImpulseResponseBank.from_taps(_rirs(), device=DEV)


def test_bank_layout(bank):
    assert bank.n_rirs == len(RIR_SPECS) and bank.spectra.shape == (len(RIR_SPECS), 16385, 2)
    assert list(bank.lengths) == [1, 97, 3940, 16124, 16384] and list(bank.dpos) == [0, 10, 40, 40, 40]


@pytest.mark.parametrize("n", NS)
def test_reverb_matches_the_reference(bank, n):
    """Every RIR length on every augmentation length, standalone (ops.reverb) and inside KA (ops.augment, other transforms off: the
    same bits)."""
    hs = _rirs()
    R = len(hs)
    x = _clips(R, n, start=n)
    xt = torch.from_numpy(x).to(DEV)
    got = ops.reverb(xt, bank, np.arange(R))
    fused = ops.augment(xt, [dict(OFF, rir=r) for r in range(R)], rirs=bank)
    assert torch.equal(got, fused)
    g = got.cpu().numpy()
    for r in range(R):
        _check(g[r], x[r], hs[r])


def test_unit_impulse_gives_the_input_back():
    h = np.zeros(500, np.float32)
    h[123] = 0.25
    b = ImpulseResponseBank.from_taps([h], device=DEV)
    assert int(b.dpos[0]) == 40 and int(b.lengths[0]) == 417
    for n in (4000, 16000, 16383, 24000):
        x = _clips(3, n, start=7)
        got = ops.reverb(torch.from_numpy(x).to(DEV), b, 0).cpu().numpy()
        assert np.abs(got - x).max() <= TOL * np.abs(x).max(axis=1).max()


@pytest.mark.parametrize("n", (16000, 8000))
def test_energy_is_preserved(bank, n):
    x = _clips(5, n, start=3)
    got = ops.reverb(torch.from_numpy(x).to(DEV), bank, np.arange(5)).cpu().numpy().astype(np.float64)
    ex = (x.astype(np.float64) ** 2).sum(axis=1)
    assert np.abs((got ** 2).sum(axis=1) / ex - 1).max() <= 1e-6


def test_two_block_lengths_match_the_reference(bank):
    hs = _rirs()
    for n in (24000, 32000):
        x = _clips(len(hs), n, start=n)
        got = ops.reverb(torch.from_numpy(x).to(DEV), bank, np.arange(len(hs))).cpu().numpy()
        for r in range(len(hs)):
            _check(got[r], x[r], hs[r])


def test_silence_and_negative_index(bank):
    x = _clips(3, 16000, start=1)
    x[1] = 0.0
    xt = torch.from_numpy(x).to(DEV)
    got = ops.reverb(xt, bank, [-1, 2, -5])
    assert torch.equal(got[0], xt[0]) and torch.equal(got[1], xt[1]) and torch.equal(got[2], xt[2])


def test_results_do_not_depend_on_the_batch(bank):
    n = 16000
    B = 4096
    rng = np.random.default_rng(5)
    x = torch.from_numpy(pkg.synth.make_clips_tiled(0, B, unique=64, n=n)).to(DEV)
    idx = rng.integers(-1, bank.n_rirs, B)
    full = ops.reverb(x, bank, idx)
    for lo, m in ((0, 1), (100, 37), (4059, 37)):
        assert torch.equal(ops.reverb(x[lo:lo + m], bank, idx[lo:lo + m]), full[lo:lo + m])
    perm = rng.permutation(B)
    assert torch.equal(ops.reverb(x[perm], bank, idx[perm]), full[perm])
    plans = [dict(OFF, rir=int(i)) if i >= 0 else dict(OFF) for i in idx]
    fused = ops.augment(x, plans, rirs=bank)
    assert torch.equal(fused, full)
    assert torch.equal(ops.augment(x[perm], [plans[i] for i in perm], rirs=bank), full[perm])


def _noise_bank():
    rng = np.random.default_rng(3)
    files = [(rng.standard_normal(m) * 0.2).astype(np.float32) for m in (30000, 2000, 900)]
    return BackgroundNoiseBank.from_buffer(torch.from_numpy(np.concatenate(files)).to(DEV), [len(f) for f in files])


def _draw(rng, n, B, p_bg, p_rir, bgbank, R):
    plans = []
    for _ in range(B):
        p = ao.draw_plan(rng, n=n)
        if bgbank is not None and rng.random() < p_bg:
            f = rng.randrange(bgbank.n_files)
            p.update(bg_file=f, bg_start=rng.randrange(int(bgbank.lengths[f])), snr_db=rng.uniform(-5, 40))
        if rng.random() < p_rir:
            p["rir"] = rng.randrange(R)
        plans.append(p)
    return plans


@pytest.mark.parametrize("n", (16000, 12345))
def test_clips_without_reverb_keep_their_bits(bank, n):
    """In a batch where some clips reverberate, the others equal ops.augment without an RIR bank bit for bit, with and without
    background; and a batch where no clip reverberates equals it whole, through the C call with every enabled = 0 too."""
    B = 24
    bgbank = _noise_bank()
    x = torch.from_numpy(_clips(B, n, start=60)).to(DEV)
    rng = random.Random(n)
    for bgb in (None, bgbank):
        plans = _draw(rng, n, B, 0.8, 0.5, bgb, bank.n_rirs)
        got = ops.augment(x, plans, bank=bgb, rirs=bank)
        want = ops.augment(x, [{k: v for k, v in p.items() if k != "rir"} for p in plans], bank=bgb)
        off = [i for i, p in enumerate(plans) if "rir" not in p]
        on = [i for i, p in enumerate(plans) if "rir" in p]
        assert off and on
        assert torch.equal(got[off], want[off])
        assert not torch.equal(got[on], want[on])
        none = [{k: v for k, v in p.items() if k != "rir"} for p in plans]
        assert torch.equal(ops.augment(x, none, bank=bgb, rirs=bank), want)
        # the C call with every enabled = 0
        ref = ops.augment(x, none, bank=bgb)
        plans_c = _plan_array(none)
        bg = ops._bg_array(none, bgb, B) if bgb is not None else None
        rir = (nat.AugmentRir * B)()
        out = torch.empty_like(x)
        ws = torch.empty(int(nat.lib.ww_augment_rir_workspace_bytes(B, n)), dtype=torch.uint8, device=DEV)
        xa = ops._aligned_rows(x)                                           # (rows of a multiple of 4 floats, as ops.augment passes them)
        nat.check(nat.lib.ww_augment_rir_f32(xa.data_ptr(), B, xa.stride(0), n, plans_c, bg, bgb.data.data_ptr() if bgb is not None else None,
                                             bgb.data.numel() if bgb is not None else 0, rir, bank.spectra.data_ptr(), bank.n_rirs,
                                             out.data_ptr(), n, ws.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        assert torch.equal(out, ref)


def _plan_array(plans):
    """ops.augment's conversion of dict plans to ww_augment_plan records."""
    arr = (nat.AugmentPlan * len(plans))()
    for i, p in enumerate(plans):
        a = arr[i]
        a.shift = int(p.get("shift", 0))
        a.crop_start = int(p.get("crop", 0))
        n_steps = p.get("n_steps")
        a.pitch_rate = float(p["pitch_rate"]) if p.get("pitch_rate") else (2.0 ** (-float(n_steps) / 12.0) if n_steps is not None else 0.0)
        a.stretch_rate = float(p["rate"]) if p.get("rate") else 0.0
        a.noise_sigma = float(p.get("sigma", 0.0))
        a.noise_seed = int(p.get("seed", 0)) & 0xFFFFFFFF
    return arr


@pytest.mark.parametrize("n", (16000, 8000))
def test_records_path_is_graph_capturable_and_bitwise_equal(bank, n):
    """ww_augment_rir_prepare + ww_augment_rir_records_f32 captured once and replayed with new records: every replay equals the direct
    call (ops.augment with both banks), batches without any reverb or background included."""
    B = 10
    x = torch.from_numpy(_clips(B, n, start=40)).to(DEV)
    bgbank = _noise_bank()
    rb = int(nat.lib.ww_augment_rir_record_bytes())
    rec_host = torch.empty(B * rb, dtype=torch.uint8).pin_memory()
    rec_dev = torch.empty(B * rb, dtype=torch.uint8, device=DEV)
    out = torch.empty_like(x)
    ws = torch.empty(int(nat.lib.ww_augment_rir_workspace_bytes(B, n)), dtype=torch.uint8, device=DEV)
    rng = random.Random(78)
    batches = [_draw(rng, n, B, 0.8, 0.5, bgbank, bank.n_rirs), _draw(rng, n, B, 1.0, 1.0, bgbank, bank.n_rirs),
               _draw(rng, n, B, 0.0, 0.5, bgbank, bank.n_rirs), _draw(rng, n, B, 0.0, 0.0, bgbank, bank.n_rirs)]

    def prepare(plans):
        bg = ops._bg_array(plans, bgbank, B)
        rir = ops._rir_array(plans, bank, B)
        nat.check(nat.lib.ww_augment_rir_prepare(C.cast(_plan_array(plans), C.c_void_p), C.cast(bg, C.c_void_p), C.cast(rir, C.c_void_p),
                                                 B, n, bgbank.data.numel(), bank.n_rirs, C.c_void_p(rec_host.data_ptr())))

    def launch(stream):
        nat.check(nat.lib.ww_augment_rir_records_f32(x.data_ptr(), B, n, n, rec_dev.data_ptr(), bgbank.data.data_ptr(), bgbank.data.numel(),
                                                     bank.spectra.data_ptr(), bank.n_rirs, out.data_ptr(), n, ws.data_ptr(),
                                                     C.c_void_p(stream.cuda_stream)))
    ops.init()
    prepare(batches[0])
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
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
        want = ops.augment(x, plans, bank=bgbank, rirs=bank)
        assert torch.equal(out, want)
    assert torch.equal(out, ops.augment(x, batches[-1]))


@pytest.mark.parametrize("n", (4000, 16000))
def test_families_share_the_staging_slots(n):
    """Plain, background and reverb calls stage their records through the same two pinned slots per device.  Six calls back to back on
    one stream without a synchronise in between (the third grows its slot, if nothing larger ran in the process before, while earlier
    copies may still be in flight) give what each gives alone; and a batch without background or reverb gives the same bits through
    every direct entry point."""
    rng = np.random.default_rng(8)
    files = [(rng.standard_normal(m) * 0.2).astype(np.float32) for m in (5000, 700)]
    bgbank = BackgroundNoiseBank.from_buffer(torch.from_numpy(np.concatenate(files)).to(DEV), [len(f) for f in files])
    rirs = ImpulseResponseBank.from_taps([reverb_ref.decaying_rir(L, d, seed=L) for L, d in ((300, 5), (6000, 80))], device=DEV)
    x = torch.from_numpy(_clips(5, n, start=20)).to(DEV)
    prng = random.Random(n)
    calls = [(B, _draw(prng, n, B, p_bg, p_rir, bgbank, rirs.n_rirs)) for B, p_bg, p_rir in
             ((2, 0.0, 0.0), (2, 1.0, 0.0), (5, 1.0, 1.0), (2, 0.0, 0.0), (2, 1.0, 0.0), (5, 1.0, 1.0))]
    assert calls[0][1] != calls[3][1] and calls[1][1] != calls[4][1] and calls[2][1] != calls[5][1]
    together = [ops.augment(x[:B], plans, bank=bgbank, rirs=rirs) for B, plans in calls]
    torch.cuda.synchronize()
    for (B, plans), got in zip(calls, together):
        alone = ops.augment(x[:B], plans, bank=bgbank, rirs=rirs)
        torch.cuda.synchronize()
        assert torch.equal(got, alone)

    B = 3
    plans = _draw(prng, n, B, 0.0, 0.0, None, 0)
    want = ops.augment(x[:B], plans)
    xa = ops._aligned_rows(x[:B])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(int(nat.lib.ww_augment_rir_workspace_bytes(B, n)), dtype=torch.uint8, device=DEV)
    bg_off, rir_off = (nat.AugmentBg * B)(), (nat.AugmentRir * B)()
    outs = [torch.empty_like(want) for _ in range(3)]
    nat.check(nat.lib.ww_augment_n_f32(xa.data_ptr(), B, xa.stride(0), n, _plan_array(plans), outs[0].data_ptr(), n, ws.data_ptr(), stream))
    nat.check(nat.lib.ww_augment_bg_f32(xa.data_ptr(), B, xa.stride(0), n, _plan_array(plans), bg_off, bgbank.data.data_ptr(),
                                        bgbank.data.numel(), outs[1].data_ptr(), n, ws.data_ptr(), stream))
    nat.check(nat.lib.ww_augment_rir_f32(xa.data_ptr(), B, xa.stride(0), n, _plan_array(plans), None, None, 0, rir_off,
                                         rirs.spectra.data_ptr(), rirs.n_rirs, outs[2].data_ptr(), n, ws.data_ptr(), stream))
    torch.cuda.synchronize()
    for out in outs:
        assert torch.equal(out, want)


def _float_wav(samples, rate):
    raw = np.asarray(samples, "<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, 1, rate, rate * 4, 4, 32)
    return b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt + b"data" + \
        struct.pack("<I", len(raw)) + raw


def test_bank_from_wav_and_flac_files_equals_load_audio(tmp_path):
    """16 kHz and 48 kHz WAV and FLAC RIRs: dpos and lengths equal those of load_audio(path) + the trimming rule, and so do the
    reverb outputs (within the tolerance); an all-zero file, a non-finite file and an unreadable file are skipped and counted."""
    specs = [("a.wav", 16000, 6000, 200), ("b.flac", 16000, 20000, 900), ("c.wav", 48000, 3 * 9000, 3 * 150),
             ("d.flac", 48000, 3 * 7000, 3 * 60)]
    paths = []
    for k, (name, rate, length, pre) in enumerate(specs):
        h = reverb_ref.decaying_rir(length, pre, seed=k, rt_samples=rate / 8)
        ints = np.round(h * 20000).astype(np.int64)
        data = flacenc.encode(ints, rate, 16) if name.endswith(".flac") else flacenc.wav_bytes(ints, rate, 16)
        p = tmp_path / name
        p.write_bytes(data)
        paths.append(str(p))
    (tmp_path / "e_zero.wav").write_bytes(flacenc.wav_bytes(np.zeros(3000, np.int64), 16000, 16))
    bad = np.zeros(3000, np.float32)
    bad[100] = np.nan
    (tmp_path / "f_nan.wav").write_bytes(_float_wav(bad, 16000))
    (tmp_path / "g_broken.wav").write_bytes(b"RIFF\x00\x00\x00\x00WAVEjunk")
    b = ImpulseResponseBank(str(tmp_path), device=DEV)
    assert b.n_rirs == 4 and b.skipped == 3 and b.stats["files"] == 4
    proc = AudioProcessor()
    loaded = [proc.load_audio(p) for p in paths]
    ref = ImpulseResponseBank.from_taps(loaded, device=DEV)
    assert np.array_equal(b.dpos, ref.dpos) and np.array_equal(b.lengths, ref.lengths)
    for h, L, d in zip(loaded, b.lengths, b.dpos):
        kept, dpos = reverb_ref.trim(h)
        assert (kept.size, dpos) == (L, d)
    x = _clips(4, 16000, start=9)
    got = ops.reverb(torch.from_numpy(x).to(DEV), b, np.arange(4)).cpu().numpy()
    want = ops.reverb(torch.from_numpy(x).to(DEV), ref, np.arange(4)).cpu().numpy()
    for r in range(4):
        assert np.abs(got[r] - want[r]).max() <= TOL * np.abs(want[r]).max()
        _check(got[r], x[r], loaded[r])
    with pytest.raises(ValueError):
        ImpulseResponseBank([str(tmp_path / "e_zero.wav")], device=DEV)


def _write_set(tmp_path, n_files, n, start):
    clips = pkg.synth.make_clips(start, n_files, n=n) * 0.8
    paths = []
    for i in range(n_files):
        p = str(tmp_path / f"c{start + i:04d}.wav")
        pkg.synth.write_wav16(p, clips[i])
        paths.append(p)
    return paths


@pytest.mark.parametrize("duration", (1.0, 0.5))
def test_training_epoch_with_rir_and_background_banks(tmp_path, duration):
    """WAV files -> WakewordDataset(augment=True) -> the package DataLoader -> model.train(): the epoch reverberates about half the
    clips, repeats bit for bit under the same seeds, and differs without the RIR bank; the per-item path uses the bank too."""
    cfg = type("Cfg", (AudioConfig,), {"DURATION": duration})
    n = int(16000 * duration)
    paths = _write_set(tmp_path, 12, n, start=700)
    rir_dir = tmp_path / "rirs"
    rir_dir.mkdir()
    for i, (L, d) in enumerate(((8000, 100), (20000, 300), (500, 5))):
        pkg.synth.write_wav16(str(rir_dir / f"rir_{i}.wav"), reverb_ref.decaying_rir(L, d, seed=i) * 0.9)
    noise_dir = tmp_path / "noise"
    noise_dir.mkdir()
    pkg.synth.write_wav16(str(noise_dir / "n0.wav"), (np.random.default_rng(1).standard_normal(30000) * 0.1).astype(np.float32))
    proc = AudioProcessor(cfg)
    proc.set_background_noise(str(noise_dir))
    rb = proc.set_room_impulse_responses(str(rir_dir))
    assert rb is proc.room_impulse_responses and rb.n_rirs == 3
    ds = pkg.WakewordDataset(paths[:6], paths[6:], proc, augment=True, verbose=False)
    T = 1 + n // 512
    data, _ = ds[0]
    assert data.shape == (1, 80, T) and torch.isfinite(data).all()
    seen = []
    orig = ops.augment

    def spy(pcm, plans, bank=None, rirs=None):
        seen.append((sum("rir" in p for p in plans), rirs))
        return orig(pcm, plans, bank=bank, rirs=rirs)
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
        for data, target in pkg.DataLoader(ds, batch_size=4, shuffle=True):
            assert data.shape[1:] == (1, 80, T) and torch.isfinite(data).all()
            batches.append(data.clone())
            opt.zero_grad()
            loss = crit(model(data), target.reshape(-1).long().to(DEV))
            loss.backward()
            opt.step()
            assert torch.isfinite(loss)
        return batches, [p.detach().clone() for p in model.parameters()]
    ops.augment = spy
    try:
        b1, p1 = epoch(5)
    finally:
        ops.augment = orig
    assert len(b1) == 3 and sum(k for k, _ in seen) >= 2 and all(r is rb for _, r in seen)
    b2, p2 = epoch(5)
    assert all(torch.equal(a, b) for a, b in zip(b1, b2)) and all(torch.equal(a, b) for a, b in zip(p1, p2))
    proc.set_room_impulse_responses(None)
    assert proc.room_impulse_responses is None
    b3, _ = epoch(5)
    assert any(not torch.equal(a, b) for a, b in zip(b1, b3))
