"""Streaming at window lengths of 0.25 .. 1 s (N = 4,000 .. 16,383 samples, T = 8 .. 32 frames): the per-hop hipGraph runs the log-mel
kernels in ring form at length N, then the conv stack at width T and the head.  Every checked hop is compared with the windowed oracle
and, bit for bit, with model.forward_pcm on the same windows at the same batch size (the same kernel instances, only the load
addressing differs)."""
import ctypes as C

import numpy as np
import pytest
import torch

import wakeword_jupyterlab_amd as pkg
from oracle import mel_oracle, model_oracle
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import ops
from wakeword_jupyterlab_amd.config import AudioConfig, n_samples
from wakeword_jupyterlab_amd.model import save_deployment_package

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3


def _cfg(n):
    cfg = type(f"AudioConfig{n}", (AudioConfig,), {"DURATION": n / 16000.0})
    assert n_samples(cfg) == n
    return cfg


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


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    return torch.device("cuda", 0)


def _model(arch, sd, dev, n):
    m = pkg.SimpleWakewordModel(audio_config=_cfg(n)) if arch == "simple" else pkg.WakewordModel(audio_config=_cfg(n))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).eval()


def _streams(n_mics, total, seed):
    """n_mics synthetic signals of `total` samples, each its own."""
    per = -(-total // 16000)
    return np.stack([np.concatenate([pkg.synth.make_clip(seed + 10 * i + j) for j in range(per)])[:total]
                     for i in range(n_mics)]).astype(np.float32)


def _window(streams, done, n):
    """The last n samples before `done`, left-padded with zeros while the window is not yet full."""
    win = np.zeros((streams.shape[0], n), np.float32)
    seg = streams[:, max(0, done - n):done]
    win[:, n - seg.shape[1]:] = seg
    return win


def _softmax1(logits):
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True))[:, 1]


def _check_hop(det, m, sd, win, oracle_rows, threshold):
    """window, oracle, forward_pcm bit for bit, prob against the logits, detections against prob."""
    det.stream.synchronize()
    n = win.shape[1]
    assert np.array_equal(det.window().cpu().numpy(), win)
    got = det.logits.cpu().numpy()
    prob = det.prob.cpu().numpy()
    with torch.no_grad():
        direct = m.forward_pcm(torch.from_numpy(win).to(det.device)).cpu().numpy()
    assert np.array_equal(got, direct), np.abs(got - direct).max()
    if len(oracle_rows):
        ref = model_oracle.forward_np(_oracle_mel(win[oracle_rows], n, True), sd)
        assert np.abs(got[oracle_rows] - ref).max() <= LOGIT_TOL, np.abs(got[oracle_rows] - ref).max()
    assert np.isfinite(prob).all() and np.abs(prob - _softmax1(got)).max() <= 1e-5
    assert np.array_equal(det.detections().cpu().numpy(), prob >= threshold)


@pytest.mark.parametrize("arch", ["simple", "full"])
@pytest.mark.parametrize("n,hop", [(4000, 160), (8000, 160), (8000, 400), (12000, 160), (15920, 80)])
def test_streaming_n_matches_oracle_and_forward_pcm(dev, arch, n, hop):
    sd = pkg.synth.make_state_dict(arch, seed=1234)
    m = _model(arch, sd, dev, n)
    n_mics, fill = 4, n // hop
    n_hops = fill + 23
    streams = _streams(n_mics, n_hops * hop, 500)
    det = pkg.StreamingDetector(m, n_mics=n_mics, hop_samples=hop, threshold=0.5)
    assert det.window_samples == n
    checks = {fill // 4, fill // 2, fill - 1, fill, fill + 10, n_hops - 1}
    for k in range(n_hops):
        det.step(torch.from_numpy(streams[:, k * hop:(k + 1) * hop]).to(dev))
        if k in checks:
            _check_hop(det, m, sd, _window(streams, (k + 1) * hop, n), np.arange(n_mics), 0.5)
    det.close()


@pytest.mark.parametrize("arch", ["simple", "full"])
@pytest.mark.parametrize("n_mics", [1, 5])
@pytest.mark.parametrize("n", [4000, 16000])
def test_streamer_step_is_the_forward_chain_on_its_window(dev, arch, n_mics, n):
    """The streamer shares its workspace layout and launch chain with the batch entry points: every hop until the ring is full, its
    logits are, bit for bit, those of the batch call on the rows ww_streamer_window unrolls -- ops.forward_pcm at one second,
    ops.forward_pcm_frames below.  One microphone (its stride is never used) and five (an odd batch)."""
    sd = pkg.synth.make_state_dict(arch, seed=1234)
    m = _model(arch, sd, dev, n)
    hop = n // 10
    streams = torch.from_numpy(_streams(n_mics, n, 900)).to(dev)
    det = pkg.StreamingDetector(m, n_mics=n_mics, hop_samples=hop)
    assert det.window_samples == n
    packed = m.packed_weights()
    for k in range(10):
        det.step(streams[:, k * hop:(k + 1) * hop])
        rows = det.window()                                            # waits for the detector's stream
        assert torch.equal(rows[:, n - (k + 1) * hop:], streams[:, :(k + 1) * hop]) and not rows[:, :n - (k + 1) * hop].any()
        direct = ops.forward_pcm(rows, packed, m._n_conv) if n == 16000 else ops.forward_pcm_frames(rows, packed, m._n_conv, n)
        assert torch.equal(det.logits.view(torch.int32), direct.view(torch.int32)), (k, det.logits, direct)
    det.close()


@pytest.mark.parametrize("conv", ["f32", "f16x3", "f16x3d"])
@pytest.mark.parametrize("mel", ["f32", "f64", "auto"])
def test_streaming_n_arithmetics(dev, conv, mel):
    """Every conv and log-mel arithmetic in the captured graph.  Microphone 0 carries a noise-free tone: in auto mode its windows sit
    on the float FFT's rounding floor, so the ring-form float64 redo at the 64-frame tile runs (it is compared with the oracle in the
    f64 and auto modes; the plain float32 front end is not held to the oracle on it)."""
    n, hop, n_hops = 8000, 400, 27
    sd = pkg.synth.make_state_dict("simple", seed=1234)
    m = _model("simple", sd, dev, n)
    t = np.arange(n_hops * hop) / 16000.0
    streams = np.concatenate([(0.5 * np.sin(2 * np.pi * 440.0 * t))[None].astype(np.float32), _streams(2, n_hops * hop, 700)])
    ops.set_conv_math(conv)
    ops.set_logmel_math(mel)
    try:
        det = pkg.StreamingDetector(m, n_mics=3, hop_samples=hop, threshold=0.5)
        for k in range(n_hops):
            det.step(torch.from_numpy(streams[:, k * hop:(k + 1) * hop]).to(dev))
            if k in (9, 19, n_hops - 1):
                rows = np.arange(3) if mel != "f32" else np.arange(1, 3)
                _check_hop(det, m, sd, _window(streams, (k + 1) * hop, n), rows, 0.5)
        det.close()
    finally:
        ops.set_conv_math("f16x3")
        ops.set_logmel_math("auto")


def test_streaming_n_more_microphones_than_cus(dev):
    """300 microphones at N = 8,000: the 4-wave ring form, workgroups looping over microphones.  A subset against the oracle, every
    microphone bit for bit against forward_pcm at batch 300."""
    n, hop, n_mics = 8000, 400, 300
    n_hops = n // hop + 6
    sd = pkg.synth.make_state_dict("simple", seed=1234)
    m = _model("simple", sd, dev, n)
    base = _streams(20, n_hops * hop, 900)
    streams = np.stack([np.roll(base[i % 20], 53 * i) * (1.0 + i / n_mics) for i in range(n_mics)]).astype(np.float32)
    det = pkg.StreamingDetector(m, n_mics=n_mics, hop_samples=hop, threshold=0.5)
    for k in range(n_hops):
        det.step(torch.from_numpy(streams[:, k * hop:(k + 1) * hop]).to(dev))
        if k in (7, n // hop - 1, n_hops - 1):
            _check_hop(det, m, sd, _window(streams, (k + 1) * hop, n), np.arange(3, n_mics, 23), 0.5)
    det.close()


def test_streaming_n_silence_is_nan_and_never_detected(dev):
    n, hop = 4000, 160
    sd = pkg.synth.make_state_dict("simple", seed=1234)
    m = _model("simple", sd, dev, n)
    streams = _streams(2, 40 * hop, 40)
    streams[1] = 0.0                                       # a dead microphone
    det = pkg.StreamingDetector(m, n_mics=2, hop_samples=hop, threshold=0.0)
    for k in range(40):
        det.step(torch.from_numpy(streams[:, k * hop:(k + 1) * hop]).to(dev))
    det.stream.synchronize()
    win = _window(streams, 40 * hop, n)
    assert np.array_equal(det.window().cpu().numpy(), win)
    prob, got = det.prob.cpu().numpy(), det.logits.cpu().numpy()
    assert np.isnan(prob[1]) and np.isfinite(prob[0])
    assert det.detections().cpu().numpy().tolist() == [True, False]      # threshold 0: every finite probability detects, NaN never
    with torch.no_grad():
        direct = m.forward_pcm(torch.from_numpy(win).to(dev)).cpu().numpy()
    assert np.array_equal(got, direct, equal_nan=True)
    det.close()


class _Raw1s:
    """The 1 s entry point ww_streamer_create, driven directly."""

    def __init__(self, m, n_mics, hop, dev):
        self.packed = m.packed_weights()
        self.stream = torch.cuda.Stream(device=dev)
        self.prob = torch.zeros(n_mics, device=dev)
        self.logits = torch.zeros((n_mics, 2), device=dev)
        self.hop_buf = torch.zeros((n_mics, hop), device=dev)
        h = C.c_void_p()
        nat.check(nat.lib.ww_streamer_create(n_mics, hop, C.c_void_p(self.packed.data_ptr()), m._n_conv,
                                             C.c_void_p(self.stream.cuda_stream), C.byref(h)))
        self.h = h

    def step(self, hop):
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            self.hop_buf.copy_(hop)
        nat.check(nat.lib.ww_streamer_step(self.h, C.c_void_p(self.hop_buf.data_ptr()), C.c_void_p(self.prob.data_ptr()),
                                           C.c_void_p(self.logits.data_ptr())))

    def close(self):
        self.stream.synchronize()
        nat.lib.ww_streamer_destroy(self.h)


def test_one_second_create_n_is_create(dev):
    """ww_streamer_create_n(..., 16000, ...) (what StreamingDetector calls) and ww_streamer_create: bitwise identical over 120 hops."""
    n_mics, hop, n_hops = 64, 160, 120
    sd = pkg.synth.make_state_dict("simple", seed=1234)
    m = _model("simple", sd, dev, 16000)
    streams = torch.from_numpy(_streams(n_mics, n_hops * hop, 1100)).to(dev)
    det = pkg.StreamingDetector(m, n_mics=n_mics, hop_samples=hop)
    assert det.window_samples == 16000
    raw = _Raw1s(m, n_mics, hop, dev)
    for k in range(n_hops):
        chunk = streams[:, k * hop:(k + 1) * hop]
        det.step(chunk)
        raw.step(chunk)
        det.stream.synchronize()
        raw.stream.synchronize()
        assert torch.equal(det.logits, raw.logits) and torch.equal(det.prob, raw.prob), k
    assert torch.isfinite(det.prob).all()
    det.close()
    raw.close()


def test_streaming_n_repeats_bit_for_bit(dev):
    n, hop, n_hops = 8000, 160, 70
    sd = pkg.synth.make_state_dict("full", seed=99)
    m = _model("full", sd, dev, n)
    streams = torch.from_numpy(_streams(8, n_hops * hop, 1300)).to(dev)
    a = pkg.StreamingDetector(m, n_mics=8, hop_samples=hop)
    b = pkg.StreamingDetector(m, n_mics=8, hop_samples=hop)
    for k in range(n_hops):
        a.step(streams[:, k * hop:(k + 1) * hop])
        b.step(streams[:, k * hop:(k + 1) * hop])
        a.stream.synchronize()
        b.stream.synchronize()
        assert torch.equal(a.logits, b.logits) and torch.equal(a.prob, b.prob), k
    a.close()
    b.close()


def test_train_package_stream_at_half_a_second(dev, tmp_path):
    """Train a 0.5 s SimpleWakewordModel for a few steps, save the deployment package, rebuild the model from the package's
    audio_config, load the weights and stream: each checked hop's probability is the softmax of forward_pcm on that window."""
    cfg = _cfg(8000)
    torch.manual_seed(0)
    model = pkg.SimpleWakewordModel(audio_config=cfg).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    crit = torch.nn.CrossEntropyLoss()
    x = torch.from_numpy(pkg.synth.make_clips(200, 8, n=8000)).to(dev)
    y = torch.tensor([0, 1] * 4, device=dev)
    mel = ops.logmel_frames(x, 8000, True)
    assert mel.shape == (8, 1, 80, 16)
    before = [p.detach().clone() for p in model.parameters()]
    for _ in range(4):
        opt.zero_grad()
        loss = crit(model(mel), y)
        loss.backward()
        opt.step()
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
    path = str(tmp_path / "half.pth")
    save_deployment_package(model.eval(), path)
    saved = torch.load(path, weights_only=True)
    assert saved["audio_config"]["DURATION"] == 0.5
    rebuilt = pkg.SimpleWakewordModel(audio_config=type("Deployed", (AudioConfig,), dict(saved["audio_config"])))
    rebuilt.load_state_dict(saved["model_state_dict"])
    rebuilt = rebuilt.to(dev).eval()
    assert rebuilt._n_samples == 8000

    hop, n_hops = 160, 80
    streams = _streams(6, n_hops * hop, 1500)
    det = pkg.StreamingDetector(rebuilt, n_mics=6, hop_samples=hop)
    assert det.window_samples == 8000
    for k in range(n_hops):
        det.step(torch.from_numpy(streams[:, k * hop:(k + 1) * hop]).to(dev))
        if k in (20, 49, 50, n_hops - 1):
            det.stream.synchronize()
            win = _window(streams, (k + 1) * hop, 8000)
            assert np.array_equal(det.window().cpu().numpy(), win)
            with torch.no_grad():
                lg = rebuilt.forward_pcm(torch.from_numpy(win).to(dev))
            assert torch.equal(det.logits, lg)
            want = (1.0 / (1.0 + torch.exp(lg[:, 0] - lg[:, 1]))).cpu().numpy()     # softmax(logits)[1], as the head writes it
            got = det.prob.cpu().numpy()
            assert np.array_equal(got, want), np.abs(got - want).max()
            assert np.abs(got - torch.softmax(lg, dim=1)[:, 1].cpu().numpy()).max() <= 1e-6
    det.close()
