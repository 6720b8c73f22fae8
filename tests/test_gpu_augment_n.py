"""KA at clip lengths of 4,000 .. 16,383 samples (DURATION 0.25 .. 1 s, T <= 32 frames) on the GPU, against oracle/augment_oracle.py at
the same length, and the training flow it opens: WAV files -> WakewordDataset(augment=True) -> DataLoader -> train-mode model.

Tolerances are tests/test_gpu_augment.py's (see its header): time shift exact, noise 1e-6, max |err| <= 3e-3 of the clip's peak and
rms err <= 1e-3 of its rms per vocoder pass, twice that for pitch + stretch."""
import copy
import ctypes as C
import random

import numpy as np
import pytest
import torch

import wakeword_jupyterlab_amd as pkg
from oracle import augment_oracle as ao
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import ops
from wakeword_jupyterlab_amd.audio import AudioProcessor
from wakeword_jupyterlab_amd.config import AudioConfig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OFF = {"shift": 0, "n_steps": None, "rate": None, "crop": 0, "sigma": 0.0, "seed": 0}
NS = (4000, 5001, 8000, 12345, 15872, 16000, 16383)


def _cfg(duration):
    return type("Cfg", (AudioConfig,), {"DURATION": duration})


def _clips(count, n, start=0):
    x = pkg.synth.make_clips(start, count, n=n)
    return x / np.abs(x).max(axis=1, keepdims=True)


def _run(x, plans):
    return ops.augment(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV), plans).cpu().numpy()


def _check(got, want, max_rel=3e-3, rms_rel=1e-3):
    assert got.shape == want.shape and got.dtype == np.float32
    err = got.astype(np.float64) - want.astype(np.float64)
    peak, rms = np.abs(want).max(), np.sqrt((want.astype(np.float64) ** 2).mean())
    assert np.abs(err).max() <= max_rel * peak, (np.abs(err).max() / peak)
    assert np.sqrt((err ** 2).mean()) <= rms_rel * rms, (np.sqrt((err ** 2).mean()) / rms)


def _plans_array(plans):
    arr = (nat.AugmentPlan * max(1, len(plans)))()
    for a, p in zip(arr, plans):
        a.shift, a.crop_start = p["shift"], p["crop"]
        a.pitch_rate = ao.pitch_rate(p["n_steps"]) if p["n_steps"] is not None else 0.0
        a.stretch_rate = p["rate"] or 0.0
        a.noise_sigma, a.noise_seed = p["sigma"], p["seed"]
    return arr


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("n", NS)
def test_identity_roll_and_noise(n):
    x = _clips(8, n)
    assert np.array_equal(_run(x[:3], [OFF] * 3), x[:3])
    shifts = [1, -1, 3, 4799, -4800, n - 1, n + 7, -3 * n - 5]
    got = _run(x, [dict(OFF, shift=s) for s in shifts])
    for i, s in enumerate(shifts):
        assert np.array_equal(got[i], np.roll(x[i], s)), s
    seeds = (12345, 2 ** 32 - 1)
    got = _run(x[:2], [dict(OFF, sigma=0.15, seed=s) for s in seeds])
    for i, seed in enumerate(seeds):
        want = (x[i].astype(np.float64) + 0.15 * ao.hash_normal(seed, n)).astype(np.float32)
        assert np.abs(got[i] - want).max() <= 1e-6


@pytest.mark.parametrize("n", NS)
def test_time_stretch_against_the_oracle(n):
    x = _clips(2, n, start=3)                                   # clip 3 is tonal, clip 4 noise
    for rate in (0.7, 0.91, 1.3):
        n_str = int(round(n / rate))
        crop = (n_str - n) // 3 if n_str > n else 0
        got = _run(x, [dict(OFF, rate=rate, crop=crop)] * 2)
        for i in range(2):
            z = ao.time_stretch(x[i], rate)
            want = z[crop:crop + n] if len(z) > n else np.pad(z, (0, n - len(z)))
            _check(got[i], want.astype(np.float32))
            if n_str < n:
                assert np.all(got[i][n_str:] == 0.0)            # pad_or_truncate's zero pad


@pytest.mark.parametrize("n", NS)
def test_pitch_shift_against_the_oracle(n):
    x = _clips(2, n, start=6)
    got = _run(np.concatenate([x, x]), [dict(OFF, n_steps=-2.7)] * 2 + [dict(OFF, n_steps=3.0)] * 2)
    for i in range(2):
        _check(got[i], ao.pitch_shift(x[i], -2.7))
        _check(got[2 + i], ao.pitch_shift(x[i], 3.0))


@pytest.mark.parametrize("n", NS)
def test_mixed_plans_match_the_oracle_and_do_not_depend_on_the_batch(n):
    rng = random.Random(n)
    B = 8
    x = _clips(B, n, start=20)
    plans = [ao.draw_plan(rng, n=n) for _ in range(B)]
    plans[0] = dict(OFF)
    plans[1] = dict(plans[1], n_steps=None)
    plans[2] = dict(plans[2], rate=None, crop=0)
    plans[3] = dict(plans[3], n_steps=1.5, rate=0.75, crop=(round(n / 0.75) - n))    # the largest crop
    got = _run(x, plans)
    for i in range(B):
        _check(got[i], ao.augment(x[i], plans[i]), max_rel=6e-3, rms_rel=2e-3)
    # alone, or in another batch in another order, a clip gives the same bits
    for i in (0, 3, 5):
        assert np.array_equal(_run(x[i:i + 1], plans[i:i + 1])[0], got[i])
    perm = [7, 2, 5, 0, 3]
    again = _run(x[perm], [plans[i] for i in perm])
    for j, i in enumerate(perm):
        assert np.array_equal(again[j], got[i])


def test_rows_inside_a_wider_tensor_and_odd_output_strides():
    """N = 5001: the rows sit in a [B, 5008] tensor whose tail is NaN (clip_stride > N, a multiple of 4); the output rows have a stride of
    5003 (not a multiple of 4) inside a NaN-filled buffer.  Nothing outside the rows is read or written."""
    n, B, stride, ostride = 5001, 6, 5008, 5003
    rng = random.Random(3)
    x = _clips(B, n, start=60)
    plans = [ao.draw_plan(rng, n=n) for _ in range(B)]
    want = _run(x, plans)
    wide = torch.full((B, stride), float("nan"), device=DEV)
    wide[:, :n] = torch.from_numpy(x.astype(np.float32)).to(DEV)
    got = ops.augment(wide[:, :n], plans)                          # a strided view: passed through without a copy
    assert np.array_equal(got.cpu().numpy(), want)
    out = torch.full((B * ostride + 5,), float("nan"), device=DEV)
    ws = torch.empty(nat.lib.ww_augment_n_workspace_bytes(B, n), dtype=torch.uint8, device=DEV)
    nat.check(nat.lib.ww_augment_n_f32(wide.data_ptr(), B, stride, n, _plans_array(plans), C.c_void_p(out.data_ptr() + 4), ostride,
                                       ws.data_ptr(), _stream()))
    o = out.cpu().numpy()
    rows = np.stack([o[1 + i * ostride:1 + i * ostride + n] for i in range(B)])
    assert np.array_equal(rows, want)
    gaps = np.concatenate([o[:1]] + [o[1 + i * ostride + n:1 + (i + 1) * ostride] for i in range(B)] + [o[1 + B * ostride:]])
    assert np.isnan(gaps).all()                                    # untouched
    # one clip: its stride is never used
    nat.check(nat.lib.ww_augment_n_f32(wide.data_ptr(), 1, 1, n, _plans_array(plans[:1]), out.data_ptr(), n, ws.data_ptr(), _stream()))
    assert np.array_equal(out[:n].cpu().numpy(), want[0])


def test_n_16000_is_bit_identical_to_the_one_second_calls():
    n, B = 16000, 24
    rng = random.Random(16000)
    x = torch.from_numpy(np.ascontiguousarray(_clips(B, n, start=80), dtype=np.float32)).to(DEV)
    arr = _plans_array([ao.draw_plan(rng) for _ in range(B)])
    ws = torch.empty(nat.lib.ww_augment_workspace_bytes(B), dtype=torch.uint8, device=DEV)
    assert nat.lib.ww_augment_n_workspace_bytes(B, n) == ws.numel()
    a, b, c = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    nat.check(nat.lib.ww_augment_f32(x.data_ptr(), B, n, arr, a.data_ptr(), ws.data_ptr(), _stream()))
    nat.check(nat.lib.ww_augment_n_f32(x.data_ptr(), B, n, n, arr, b.data_ptr(), n, ws.data_ptr(), _stream()))
    rb = nat.lib.ww_augment_record_bytes()
    rec = np.zeros(B * rb, np.uint8)
    nat.check(nat.lib.ww_augment_plans_prepare_n(C.cast(arr, C.c_void_p), B, n, rec.ctypes.data))
    rec_dev = torch.from_numpy(rec).to(DEV)
    nat.check(nat.lib.ww_augment_records_n_f32(x.data_ptr(), B, n, n, rec_dev.data_ptr(), c.data_ptr(), n, ws.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(ops.augment(x, arr), a)


def test_two_call_form_at_8000_is_graph_capturable_and_bitwise_equal():
    """ww_augment_plans_prepare_n + ww_augment_records_n_f32 at N = 8000, captured once with the host -> device copy of the records and
    replayed with new plans: every replay equals ww_augment_n_f32 on the same plans bit for bit, a batch without pitch included."""
    n, B = 8000, 10
    x = torch.from_numpy(np.ascontiguousarray(_clips(B, n, start=40), dtype=np.float32)).to(DEV)
    rb = int(nat.lib.ww_augment_record_bytes())
    rec_host = torch.empty(B * rb, dtype=torch.uint8).pin_memory()
    rec_dev = torch.empty(B * rb, dtype=torch.uint8, device=DEV)
    out = torch.empty_like(x)
    ws = torch.empty(int(nat.lib.ww_augment_n_workspace_bytes(B, n)), dtype=torch.uint8, device=DEV)
    rng = random.Random(78)
    batches = [[ao.draw_plan(rng, n=n) for _ in range(B)] for _ in range(3)]
    batches.append([dict(p, n_steps=None) for p in batches[0]])                       # nobody asks for pitch

    def prepare(plans):
        nat.check(nat.lib.ww_augment_plans_prepare_n(C.cast(_plans_array(plans), C.c_void_p), B, n, C.c_void_p(rec_host.data_ptr())))

    def launch(stream):
        nat.check(nat.lib.ww_augment_records_n_f32(x.data_ptr(), B, n, n, rec_dev.data_ptr(), out.data_ptr(), n, ws.data_ptr(),
                                                   C.c_void_p(stream.cuda_stream)))
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
        want = ops.augment(x, _plans_array(plans))
        assert torch.equal(out, want)


def test_audio_processor_augment_audio_at_half_a_second():
    proc = AudioProcessor(_cfg(0.5))
    y = _clips(1, 8000, start=9)[0]
    for seed in (7, 8, 9):
        random.seed(seed)
        z = proc.augment_audio(y)
        assert isinstance(z, np.ndarray) and z.shape == (8000,) and z.dtype == np.float32 and np.isfinite(z).all()
        random.seed(seed)
        plan = proc.draw_augment_plan()
        _check(z, ao.augment(y, plan), max_rel=6e-3, rms_rel=2e-3)
    with pytest.raises(ValueError):
        proc.augment_audio(y[:7999])
    with pytest.raises(ValueError):
        proc.augment_audio(np.zeros(16000, np.float32))
    assert proc.augment_batch(np.stack([y, y])).shape == (2, 8000)


def _write_set(tmp_path, n_files, n, start):
    clips = pkg.synth.make_clips(start, n_files, n=n) * 0.8
    paths = []
    for i in range(n_files):
        p = str(tmp_path / f"c{start + i:04d}.wav")
        pkg.synth.write_wav16(p, clips[i][: n - 37 * (i % 3)])                     # some files shorter than the clip: zero-padded
        paths.append(p)
    return paths


@pytest.mark.parametrize("arch", ["simple", "full"])
def test_training_flow_at_half_a_second(tmp_path, arch):
    """WAV files at DURATION 0.5 -> WakewordDataset(augment=True) -> DataLoader(batch_size=4, shuffle=True) -> train-mode model:
    [B, 1, 80, 16] batches, finite loss and gradients, optimizer steps; a seeded epoch repeats bit for bit."""
    cfg = _cfg(0.5)
    paths = _write_set(tmp_path, 10, 8000, start=300)
    proc = AudioProcessor(cfg)
    ds = pkg.WakewordDataset(paths[:4], paths[4:], proc, augment=True, verbose=False)
    data, target = ds[0]
    assert data.shape == (1, 80, 16) and target.shape == (1,) and torch.isfinite(data).all()
    torch.manual_seed(0)
    model0 = (pkg.SimpleWakewordModel(audio_config=cfg) if arch == "simple" else pkg.WakewordModel(audio_config=cfg)).to(DEV)

    def epoch(seed):
        random.seed(seed)
        torch.manual_seed(seed)
        model = copy.deepcopy(model0)
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        crit = torch.nn.CrossEntropyLoss()
        losses, shapes = [], []
        for data, target in pkg.DataLoader(ds, batch_size=4, shuffle=True, num_workers=2):
            shapes.append(tuple(data.shape))
            opt.zero_grad()
            loss = crit(model(data), target.squeeze(1))
            loss.backward()
            assert torch.isfinite(loss)
            assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
            opt.step()
            losses.append(loss.detach())
        return torch.stack(losses), shapes, [p.detach().clone() for p in model.parameters()]
    l1, shapes, p1 = epoch(5)
    assert shapes == [(4, 1, 80, 16), (4, 1, 80, 16), (2, 1, 80, 16)]
    assert any(not torch.equal(a, b) for a, b in zip(p1, model0.parameters()))         # the optimizer moved the weights
    l2, _, p2 = epoch(5)
    assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(p1, p2))
    l3, _, _ = epoch(6)
    assert not torch.equal(l1, l3)                                                      # other draws, other batches
