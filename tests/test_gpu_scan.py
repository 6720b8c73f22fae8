"""Long recordings on the MI355X: Scan.prob is the head's p(wakeword) of forward_pcm on every window,
bit for bit, and what a StreamingDetector holds after each hop; WAV and FLAC of the same integers scan alike; the sweep kernel counts
and flags events exactly as the numpy restatement (tests/events_ref.py); the detector's event flags equal Scan.events; det_curve and
hard_negatives report what the definitions say."""
import os

import numpy as np
import pytest
import torch

import events_ref
import flacenc
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import scan
from wakeword_jupyterlab_amd.config import AudioConfig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    return torch.device("cuda", 0)


def _model(arch, dev, n, seed=1234):
    cfg = type(f"AudioConfig{n}", (AudioConfig,), {"DURATION": n / 16000.0})
    sd = pkg.synth.make_state_dict(arch, seed=seed)
    m = pkg.SimpleWakewordModel(audio_config=cfg) if arch == "simple" else pkg.WakewordModel(audio_config=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).eval()


def _write(d, name, data):
    p = os.path.join(str(d), name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def _signal(n, seed, silent=0):
    """PCM-16 integers at 16 kHz: `silent` samples of zeros, then synthetic clips."""
    per = -(-max(n - silent, 0) // 16000)
    x = np.concatenate([pkg.synth.make_clip(seed + j) for j in range(per)] + [np.zeros(0, np.float32)])[:max(n - silent, 0)]
    x = np.concatenate([np.zeros(min(silent, n)), x])
    return np.clip(np.round(x * 32767), -32768, 32767).astype(np.int64)


def _wav16(d, name, ints):
    return _write(d, name, flacenc.wav_bytes(ints, 16000, 16))


def _head_prob(logits):
    """softmax(logits)[1] as the head writes it (and the streamer's prob)."""
    return (1.0 / (1.0 + torch.exp(logits[:, 0] - logits[:, 1]))).cpu().numpy()


def _materialised_prob(model, s, i, dev):
    a = s.audio[int(s.offsets[i]):int(s.offsets[i]) + int(s.lengths[i])].cpu().numpy()
    w = events_ref.windows(a, s.window, s.hop)
    if w.shape[0] == 0:
        return np.zeros(0, np.float32)
    with torch.no_grad():
        return _head_prob(model.forward_pcm(torch.from_numpy(w).to(dev)))


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("arch", ["simple", "full"])
@pytest.mark.parametrize("n", [16000, 8000, 24000])
@pytest.mark.parametrize("hop", [160, 512])
def test_scan_prob_is_forward_pcm_of_every_window(dev, tmp_path, arch, n, hop):
    m = _model(arch, dev, n)
    lens = [20803, n - 1000, hop - 60, 0, 30000]            # not a multiple of H; shorter than N; shorter than H; empty; silent start
    paths = [_wav16(tmp_path, f"f{i}.wav", _signal(L, 10 * i, silent=12000 if i == 4 else 0)) for i, L in enumerate(lens)]
    s = scan.scan_files(m, paths, hop_samples=hop)
    assert s.paths == paths and s.unreadable == [] and s.hop == hop and s.window == n
    assert s.lengths.tolist() == lens
    assert s.window_offsets.tolist() == np.concatenate([[0], np.cumsum([-(-L // hop) for L in lens])]).tolist()
    assert s.hours == pytest.approx(sum(lens) / 16000 / 3600)
    got = s.prob.cpu().numpy()
    for i in range(len(paths)):
        want = _materialised_prob(m, s, i, dev)
        assert _same(got[s.window_offsets[i]:s.window_offsets[i + 1]], want), (i, np.nanmax(np.abs(got[s.window_offsets[i]:s.window_offsets[i + 1]] - want)))
    assert np.isnan(got[s.window_offsets[4]:s.window_offsets[4] + 12000 // hop]).all()      # windows of zeros only: NaN
    s2 = scan.scan_files(m, paths, hop_samples=hop, batch_size=7)
    assert _same(s2.prob.cpu().numpy(), got)
    # the decoded audio is load_audio's
    proc = pkg.AudioProcessor()
    a = proc.load_audio(paths[0])
    assert np.array_equal(s.audio[:lens[0]].cpu().numpy(), a)


@pytest.mark.parametrize("n,arch", [(16000, "simple"), (8000, "full")])
def test_scan_matches_the_streaming_detector_hop_by_hop(dev, tmp_path, n, arch):
    """Scan.prob after every hop of a 16 kHz float mono StreamingDetector fed the decoded file (last partial hop zero-filled), bit for
    bit; with smooth / refractory_s set, its per-hop flags equal Scan.events, silent stretches included."""
    m = _model(arch, dev, n)
    hop = 160
    L = 12000 + 16000 + 12000 + 9000 + 37
    ints = np.concatenate([_signal(28000, 3, silent=12000), np.zeros(12000, np.int64), _signal(9037, 7)])
    assert ints.size == L
    path = _wav16(tmp_path, "stream.wav", ints)
    s = scan.scan_files(m, [path], hop_samples=hop)
    prob = s.prob.cpu().numpy()
    x = s.audio.cpu().numpy()
    K = -(-L // hop)
    xp = np.concatenate([x, np.zeros(K * hop - L, np.float32)])
    finite = prob[np.isfinite(prob)]
    theta = float(np.float32(np.clip(np.median(finite), 1e-3, 1.0)))
    smooth, refr = 3, 0.05
    ev_k, _ = s.events(theta, smooth=smooth, refractory_s=refr)[0]
    assert ev_k.size > 0
    det = pkg.StreamingDetector(m, n_mics=1, hop_samples=hop, threshold=theta, smooth=smooth, refractory_s=refr)
    plain = pkg.StreamingDetector(m, n_mics=1, hop_samples=hop, threshold=theta)
    fired = []
    for k in range(K):
        h = torch.from_numpy(xp[None, k * hop:(k + 1) * hop].copy()).to(dev)
        det.step(h)
        plain.step(h)
        flags = det.detections()                                  # synchronises det's stream only: plain runs on a stream of its own
        plain.stream.synchronize()
        assert _same(det.prob.cpu().numpy(), prob[k:k + 1]), k
        assert _same(plain.prob.cpu().numpy(), prob[k:k + 1]), k
        assert torch.equal(plain.detections(), plain.prob >= theta)                 # without the new arguments: today's detector
        fired.append(bool(flags[0]))
        if np.isnan(prob[max(0, k - smooth + 1):k + 1]).all():
            assert not fired[-1]                                                      # a silent stretch never fires
    assert np.isnan(prob).any()
    assert np.array_equal(np.flatnonzero(fired) + 1, ev_k)
    det.close()
    plain.close()


def test_wav_and_flac_of_the_same_integers_scan_alike(dev, tmp_path):
    m = _model("simple", dev, 16000)
    ints = flacenc.signal(44100 * 2 + 333, 2, 16, seed=5)
    w = _write(tmp_path, "a.wav", flacenc.wav_bytes(ints, 44100, 16))
    f = _write(tmp_path, "a.flac", flacenc.encode(ints, 44100, 16))
    bad = _write(tmp_path, "bad.wav", b"RIFF\x00\x00\x00\x00JUNKJUNKJUNK" * 10)
    s = scan.scan_files(m, [w, bad, f], hop_samples=512)
    assert s.paths == [w, f] and s.unreadable == [bad]
    assert s.lengths[0] == s.lengths[1] > 0
    assert s.hours == pytest.approx(2 * int(s.lengths[0]) / 16000 / 3600)
    assert np.array_equal(s.file_prob(0).cpu().numpy(), s.file_prob(1).cpu().numpy(), equal_nan=True)
    assert np.isfinite(s.file_prob(0).cpu().numpy()).all()


def _dev_scan(dev, prob, ks, hop=160):
    return scan.Scan(torch.from_numpy(np.asarray(prob, np.float32)).to(dev), [k * hop for k in ks], [f"s{i}" for i in range(len(ks))], [],
                     hop, 16000, None, dev)


@pytest.mark.parametrize("w", [1, 3, 10, 256])
def test_sweep_equals_the_restatement(dev, w):
    rng = np.random.default_rng(w)
    thr = np.linspace(0.001, 1.0, 1000).astype(np.float32)
    ks = [0, 1, 5000, 3, 0, 777, 2049, 1]                       # empty, one window, several 2048-window LDS chunks, odd starts
    total = sum(ks)
    prob = rng.random(total).astype(np.float32)
    eq = rng.random(total) < 0.3
    prob[eq] = thr[rng.integers(0, 1000, int(eq.sum()))]       # scores exactly equal to thresholds
    prob[rng.random(total) < 0.05] = np.nan
    prob[rng.random(total) < 0.01] = 1.0
    s = _dev_scan(dev, prob, ks)
    offs = s.window_offsets
    for R in (0, 1, 5, 100):
        refr = R * 160 / 16000
        assert scan.refractory_windows(refr, 160) == R
        got = s.counts(thr, smooth=w, refractory_s=refr)
        want = events_ref.counts(prob, offs, thr, w, R)
        assert got.shape == (len(ks), 1000) and got.dtype == np.int64
        assert np.array_equal(got, want), (R, np.argwhere(got != want)[:5])
        t1 = float(thr[rng.integers(0, 1000)]) if R else float(np.float32(0.5))
        ev = s.events(t1, smooth=w, refractory_s=refr)
        for g in range(len(ks)):
            seg = prob[offs[g]:offs[g + 1]]
            f = events_ref.fired(events_ref.smooth(seg, w), [t1], R)[0] if seg.size else np.zeros(0, bool)
            assert np.array_equal(ev[g][0], np.flatnonzero(f) + 1), (R, g)
            assert np.array_equal(ev[g][1], (np.flatnonzero(f) + 1) * 160 / 16000)


@pytest.mark.parametrize("R", [1, 5, 100])
def test_refractory_boundary(dev, R):
    """k - k_last = R does not fire, R + 1 does."""
    K = 3 * R + 10
    prob = np.zeros(K, np.float32)
    prob[[0, R, R + 1, 2 * R + 1, 2 * R + 2]] = 0.9
    s = _dev_scan(dev, prob, [K])
    (k, _), = s.events(0.9, smooth=1, refractory_s=R * 160 / 16000)
    assert k.tolist() == [1, R + 2, 2 * R + 3]
    assert s.counts([0.9, 0.91], smooth=1, refractory_s=R * 160 / 16000).tolist() == [[3, 0]]


def test_det_curve_and_hard_negatives(dev, tmp_path):
    m = _model("simple", dev, 8000)
    pos = [_wav16(tmp_path, f"p{i}.wav", _signal(9000 + 1234 * i, 100 + i)) for i in range(4)]
    neg = [_wav16(tmp_path, f"n{i}.wav", _signal(40000 + 777 * i, 200 + 3 * i, silent=5000 * i)) for i in range(3)]
    bad = _write(tmp_path, "n_bad.wav", b"not audio at all")
    hop, smooth, refr = 160, 3, 0.25
    c = scan.det_curve(m, pos, neg + [bad], hop_samples=hop, smooth=smooth, refractory_s=refr)
    assert c["unreadable"] == [bad] and c["n_positive"] == 4
    thr = np.linspace(0.001, 1.0, 1000).astype(np.float32)
    assert np.array_equal(c["thresholds"], thr)
    sp = scan.scan_files(m, pos, hop_samples=hop)
    sn = scan.scan_files(m, neg, hop_samples=hop)
    R = events_ref.refractory_windows(refr, hop)
    cp = events_ref.counts(sp.prob.cpu().numpy(), sp.window_offsets, thr, smooth, R)
    cn = events_ref.counts(sn.prob.cpu().numpy(), sn.window_offsets, thr, smooth, R)
    hours = sum(40000 + 777 * i for i in range(3)) / 16000 / 3600
    assert c["negative_hours"] == pytest.approx(hours)
    assert np.array_equal(c["fa_per_hour"], cn.sum(axis=0) / sn.hours)
    assert np.array_equal(c["frr"], (cp == 0).sum(axis=0) / 4)
    assert c["fa_per_hour"][0] > 0
    for target in (0.0, 1.0, float(c["fa_per_hour"][0]), float(np.median(c["fa_per_hour"]))):
        ok = np.flatnonzero(c["fa_per_hour"] <= target)
        want = float(thr[ok].min()) if ok.size else None
        assert c.threshold_for(target) == want
    # hard negatives: exactly the decoded windows that fired
    theta = float(thr[int(np.argmax(c["fa_per_hour"] <= np.median(c["fa_per_hour"])))])
    pcm, files, times = sn.hard_negatives(theta, smooth=smooth, refractory_s=refr)
    ev = sn.events(theta, smooth=smooth, refractory_s=refr)
    assert pcm.shape == (sum(k.size for k, _ in ev), 8000) and pcm.dtype == torch.float32 and pcm.device.type == "cuda"
    got = pcm.cpu().numpy()
    row = 0
    for i, (k, t) in enumerate(ev):
        a = sn.audio[int(sn.offsets[i]):int(sn.offsets[i]) + int(sn.lengths[i])].cpu().numpy()
        wins = events_ref.windows(a, 8000, hop)
        for kk, tt in zip(k, t):
            assert files[row] == i and times[row] == tt
            assert np.array_equal(got[row], wins[kk - 1])
            row += 1
    if row > 1:
        p2, f2, t2 = sn.hard_negatives(theta, smooth=smooth, refractory_s=refr, max_windows=1)
        assert p2.shape[0] == 1 and torch.equal(p2[0], pcm[0])
