"""Streaming at the microphone's own rate, sample format and channel count.  The window a detector holds after k hops is checked bit for
bit against K0's decode (AudioProcessor.load_audio) of a WAV file of the same frames -- samples [k * hop_out - D - N, k * hop_out - D),
zero-padded on the left -- and against the float64 resample_poly oracle; the logits against model.forward_pcm on that window."""
import os
import struct
from math import gcd

import numpy as np
import pytest
import torch

import wakeword_jupyterlab_amd as pkg
from oracle import decode_oracle
from wakeword_jupyterlab_amd.audio import AudioProcessor
from wakeword_jupyterlab_amd.config import AudioConfig, n_samples

pytestmark = pytest.mark.gpu

# rate -> (input frames per hop, 16 kHz samples per hop, D).  8,820 Hz: a 16,001-tap filter, too long for LDS beside the hop's frames --
# the kernel's global-memory taps (11.025 kHz's 12,801 taps, global in K0, fit in LDS here).
HOPS = {48000: (480, 160, 10), 44100: (441, 160, 10), 22050: (441, 320, 10), 11025: (441, 640, 14), 8820: (441, 800, 18),
        8000: (80, 160, 20)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    return torch.device("cuda", 0)


def _model(dev, n=16000, arch="simple"):
    cfg = type(f"AudioConfig{n}", (AudioConfig,), {"DURATION": n / 16000.0})
    assert n_samples(cfg) == n
    m = pkg.SimpleWakewordModel(audio_config=cfg) if arch == "simple" else pkg.WakewordModel(audio_config=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in pkg.synth.make_state_dict(arch, seed=1234).items()})
    return m.to(dev).eval()


def _signals(n_mics, n_frames, rate, channels, seed):
    """float64 [n_mics, n_frames, channels] in (-1, 1): a tone per mic and channel (below 4 kHz, so 8 kHz input keeps it) plus noise."""
    t = np.arange(n_frames) / rate
    out = np.empty((n_mics, n_frames, channels))
    for m in range(n_mics):
        for c in range(channels):
            s = seed + 17 * m + 5 * c
            out[m, :, c] = (0.45 * np.sin(2 * np.pi * (150 + 61 * s % 3000) * t + m) + 0.15 * np.sin(2 * np.pi * 997.0 * t * (1 + c))
                            + 0.05 * pkg.synth.normal(s, n_frames))
    return np.clip(out, -0.99, 0.99)


def _hops(x, dtype):
    """The pushed frames in the hop dtype: int16 as a PCM-16 file stores them, float32 as is."""
    if dtype == torch.int16:
        return np.round(x * 32767).astype(np.int16)
    return x.astype(np.float32)


def _write_wav(path, frames, rate):
    """frames [n, channels] int16 (PCM) or float32 (IEEE float) -> a WAV file."""
    n, ch = frames.shape
    fmt, bits = (1, 16) if frames.dtype == np.int16 else (3, 32)
    raw = frames.astype("<i2" if fmt == 1 else "<f4").tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " + struct.pack(
        "<IHHIIHH", 16, fmt, ch, rate, rate * ch * bits // 8, ch * bits // 8, bits) + b"data" + struct.pack("<I", len(raw))
    with open(path, "wb") as f:
        f.write(hdr + raw)


def _as_float(frames):
    return frames.astype(np.float32) / np.float32(32768.0) if frames.dtype == np.int16 else frames.astype(np.float32)


def _expected(tmp_path, pushed, rate, n, hop_out, k, d, proc):
    """K0's decode of a file of the pushed frames, window [k * hop_out - d - n, k * hop_out - d), and the same from the oracle."""
    end = k * hop_out - d
    k0 = np.zeros((pushed.shape[0], n), np.float32)
    ora = np.zeros((pushed.shape[0], n), np.float64)
    for m in range(pushed.shape[0]):
        path = os.path.join(str(tmp_path), f"mic{m}.wav")
        _write_wav(path, pushed[m], rate)
        sig = proc.load_audio(path)
        ref = decode_oracle.decode(_as_float(pushed[m]), rate)
        assert sig is not None and len(sig) >= end and len(ref) >= end
        lo = max(0, end - n)
        k0[m, n - (end - lo):] = sig[lo:end]
        ora[m, n - (end - lo):] = ref[lo:end]
    return k0, ora


@pytest.mark.parametrize("rate,channels,dtype", [(48000, 1, torch.int16), (44100, 2, torch.int16), (8000, 1, torch.float32),
                                                 (11025, 1, torch.int16), (8820, 1, torch.int16), (22050, 3, torch.float32)])
def test_window_is_k0s_decode_of_the_same_frames(dev, tmp_path, rate, channels, dtype):
    hop, hop_out, d = HOPS[rate]
    n, n_mics, seconds = 16000, 3, 3
    n_hops = seconds * rate // hop
    m = _model(dev, n)
    frames = _hops(_signals(n_mics, n_hops * hop, rate, channels, seed=7 + rate % 97), dtype)
    det = pkg.StreamingDetector(m, n_mics=n_mics, hop_samples=hop, sample_rate=rate, channels=channels, dtype=dtype)
    assert det.sample_rate == rate and det.latency_samples == d and det.window_samples == n
    assert det.hop_buf.dtype == dtype and tuple(det.hop_buf.shape) == ((n_mics, hop) if channels == 1 else (n_mics, hop, channels))
    proc = AudioProcessor(device=dev)
    fill = n // hop_out
    checks = {1, 2, fill // 2, fill, fill + 1, n_hops}
    for k in range(1, n_hops + 1):
        h = frames[:, (k - 1) * hop:k * hop]
        det.step(torch.from_numpy(h if channels > 1 else h[..., 0]).to(dev))
        if k in checks:
            got = det.window().cpu().numpy()
            k0, ora = _expected(tmp_path, frames[:, :k * hop], rate, n, hop_out, k, d, proc)
            assert np.array_equal(got, k0), (k, np.abs(got - k0).max())
            assert np.abs(got - ora).max() <= 1e-5, (k, np.abs(got - ora).max())
    det.close()


@pytest.mark.parametrize("n,arch", [(16000, "simple"), (8000, "full")])
def test_logits_are_forward_pcm_of_the_window(dev, n, arch):
    rate, channels, dtype = 44100, 2, torch.int16
    hop, hop_out, _ = HOPS[rate]
    n_mics = 5
    m = _model(dev, n, arch)
    n_hops = n // hop_out + 7
    frames = _hops(_signals(n_mics, n_hops * hop, rate, channels, seed=31), dtype)
    det = pkg.StreamingDetector(m, n_mics=n_mics, hop_samples=hop, threshold=0.5, sample_rate=rate, channels=channels, dtype=dtype)
    for k in range(1, n_hops + 1):
        det.step(torch.from_numpy(frames[:, (k - 1) * hop:k * hop]).to(dev))
        if k in (3, n // hop_out, n_hops):
            win = det.window()
            with torch.no_grad():
                direct = m.forward_pcm(win)
            prob = torch.softmax(direct, dim=1)[:, 1]
            det.stream.synchronize()
            assert torch.equal(det.logits, direct)
            assert torch.allclose(det.prob, prob, atol=1e-6, rtol=0)
            assert torch.equal(det.detections(), det.prob >= 0.5)
    det.close()


def _run(det, hops, dev):
    out = []
    for h in hops:
        det.step(torch.from_numpy(h).to(dev))
        det.stream.synchronize()
        out.append((det.prob.clone(), det.logits.clone()))
    return out, det.window()


def test_sixteen_khz_float_mono_is_todays_detector(dev):
    m = _model(dev)
    hop, n_mics, n_hops = 160, 4, 40
    x = _signals(n_mics, hop * n_hops, 16000, 1, seed=3)[..., 0].astype(np.float32)
    hops = [x[:, k * hop:(k + 1) * hop] for k in range(n_hops)]
    base = pkg.StreamingDetector(m, n_mics=n_mics, hop_samples=hop)
    explicit = pkg.StreamingDetector(m, n_mics=n_mics, hop_samples=hop, sample_rate=16000, dtype=torch.float32, channels=1)
    assert base.latency_samples == explicit.latency_samples == 0
    (a, wa), (b, wb) = _run(base, hops, dev), _run(explicit, hops, dev)
    for (pa, la), (pb, lb) in zip(a, b):
        assert torch.equal(la, lb) and torch.equal(pa, pb)
    assert torch.equal(wa, wb)
    # int16 at 16 kHz: the conversion alone, x / 32768
    q = np.round(x * 32767).astype(np.int16)
    as_int = pkg.StreamingDetector(m, n_mics=n_mics, hop_samples=hop, dtype=torch.int16)
    as_float = pkg.StreamingDetector(m, n_mics=n_mics, hop_samples=hop)
    assert as_int.latency_samples == 0
    (c, wc) = _run(as_int, [q[:, k * hop:(k + 1) * hop] for k in range(n_hops)], dev)
    (f, wf) = _run(as_float, [(q[:, k * hop:(k + 1) * hop].astype(np.float32) / np.float32(32768)) for k in range(n_hops)], dev)
    for (pc, lc), (pf, lf) in zip(c, f):
        assert torch.equal(lc, lf) and torch.equal(pc, pf)
    assert torch.equal(wc, wf)
    for det in (base, explicit, as_int, as_float):
        det.close()


def test_a_silent_microphone_keeps_a_zero_window(dev):
    rate, hop = 48000, 480
    n_mics, n_hops = 4, 60
    m = _model(dev)
    frames = _hops(_signals(n_mics, n_hops * hop, rate, 1, seed=11), torch.int16)[..., 0]
    frames[2] = 0
    det = pkg.StreamingDetector(m, n_mics=n_mics, hop_samples=hop, sample_rate=rate, dtype=torch.int16)
    for k in range(n_hops):
        det.step(torch.from_numpy(frames[:, k * hop:(k + 1) * hop]).to(dev))
    win = det.window().cpu().numpy()
    assert (win[2] == 0).all()
    for i in (0, 1, 3):                                           # 60 hops = 9,600 samples at 16 kHz, D = 10 of them still to come
        assert np.count_nonzero(win[i]) > 9000
    det.close()


def test_cpu_hops_and_gpu_hops_from_another_stream_agree(dev):
    rate, hop, channels = 44100, 441, 2
    n_mics, n_hops = 3, 50
    m = _model(dev)
    frames = _hops(_signals(n_mics, n_hops * hop, rate, channels, seed=19), torch.int16)
    a = pkg.StreamingDetector(m, n_mics=n_mics, hop_samples=hop, sample_rate=rate, channels=channels, dtype=torch.int16)
    b = pkg.StreamingDetector(m, n_mics=n_mics, hop_samples=hop, sample_rate=rate, channels=channels, dtype=torch.int16)
    side = torch.cuda.Stream(device=dev)
    for k in range(n_hops):
        h = frames[:, k * hop:(k + 1) * hop]
        a.step(torch.from_numpy(h))                               # a CPU tensor
        with torch.cuda.stream(side):                             # a GPU tensor made on another stream
            g = torch.from_numpy(h).to(dev, non_blocking=False) * 1
            b.step(g)
    a.stream.synchronize()
    b.stream.synchronize()
    assert torch.equal(a.window(), b.window())
    assert torch.equal(a.logits, b.logits) and torch.equal(a.prob, b.prob)
    with pytest.raises(TypeError, match="dtype"):
        a.step(torch.zeros((n_mics, hop, channels), dtype=torch.float32))
    with pytest.raises(ValueError, match="shape"):
        a.step(torch.zeros((n_mics, hop), dtype=torch.int16))
    a.close()
    b.close()


def test_latency_and_hop_table(dev):
    m = _model(dev)
    for rate, (hop, hop_out, d) in HOPS.items():
        g = gcd(16000, rate)
        assert hop * (16000 // g) == hop_out * (rate // g)
        det = pkg.StreamingDetector(m, n_mics=2, hop_samples=hop, sample_rate=rate, dtype=torch.int16)
        assert det.latency_samples == d, rate
        det.close()
