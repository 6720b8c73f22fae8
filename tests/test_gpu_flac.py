"""FLAC files through the native reader on the GPU: the frames and their index are uploaded with the staging, ww_flac.hip decodes them
to float32 and K0 takes them from there.  The contract is the WAV path's: a FLAC file gives, bit for bit, the row of the WAV file of the
same integers (x * 2^-(bps-1)), through WavBatchReader, WakewordDataset, the package's DataLoader and predict_wakeword.  The encoder is
tests/flacenc.py; with no independent FLAC implementation at hand, exactness against its integers is the oracle."""
import os
import random

import numpy as np
import pytest
import torch

import flacenc
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import files
from wakeword_jupyterlab_amd.config import AudioConfig
from wakeword_jupyterlab_amd.files import WavBatchReader

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    return torch.device("cuda", 0)


def _write(d, name, data):
    p = os.path.join(d, name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def _load(paths, normalize=True, seed=0, n_samples=16000):
    rd = WavBatchReader(max_clips=max(4, len(paths)), n_samples=n_samples)
    random.seed(seed)
    out, ok = rd.load(paths, normalize=normalize, verbose=False)
    out = out.cpu().numpy()
    rd.close()
    return out, ok


N = 12000                         # 0.75 s at 16 kHz: no crop, the row's tail is zero


def _encodings():
    """(name, samples [n] or [n, 2], bps, encode kwargs): every case of the decoder."""
    cases = []
    for bps in (8, 12, 16, 20, 24):
        x = flacenc.signal(N, 1, bps, seed=bps)[:, 0]
        cases += [(f"auto-{bps}", x, bps, {}), (f"verbatim-{bps}", x, bps, dict(subframe="verbatim")),
                  (f"rice2-{bps}", x, bps, dict(rice2=True)), (f"escape-{bps}", x, bps, dict(escape=True)),
                  (f"wasted-{bps}", x & ~7, bps, {}), (f"lpc32-{bps}", x, bps, dict(subframe="lpc", order=32, precision=15))]
        cases += [(f"fixed{o}-{bps}", x, bps, dict(subframe="fixed", order=o)) for o in range(5)]
    x = flacenc.signal(N, 1, 16, seed=1)[:, 0]
    cases += [(f"lpc{o}-p{p}", x, 16, dict(subframe="lpc", order=o, precision=p)) for o in (1, 2, 5, 8, 16, 31) for p in (2, 8, 12, 15)]
    cases += [(f"porder{p}", x[:8192], 16, dict(blocksize=4096, partition_order=p)) for p in range(9)]
    cases += [(f"porder{p}-rice2-esc", x[:8192], 16, dict(blocksize=4096, partition_order=p, rice2=True, escape=True)) for p in (0, 3, 8)]
    cases += [("constant", np.full(N, -1234), 16, dict(subframe="constant")),
              ("zeros-escape", np.zeros(N, np.int64), 16, dict(subframe="fixed", escape=True))]
    for bs in (192, 576, 1152, 2304, 4608, 256, 1024, 4096, 16, 300, 1000, 5000):
        cases.append((f"bs{bs}", x, 16, dict(blocksize=bs)))
    cases += [("bs-explicit", x, 16, dict(blocksize=4096, explicit_blocksize=True)),
              ("variable", x, 16, dict(variable=[4096, 192, 5000, 2000, 712])),
              ("explicit-rate-codes", x, 16, dict(explicit_rate=True, bps_from_streaminfo=True)),
              ("total0", x, 16, dict(total_samples_zero=True)),
              ("metadata-id3", x, 16, dict(metadata=[(1, bytes(3000)), (4, b"\x01\0\0\0v\0\0\0\0"), (6, bytes(80000))], id3=700))]
    return cases


def test_every_encoding_decodes_to_its_integers_bit_for_bit(dev, tmp_path):
    cases = _encodings()
    paths = [_write(tmp_path, f"{i}.flac", flacenc.encode(x, 16000, bps, **kw)) for i, (_, x, bps, kw) in enumerate(cases)]
    out, ok = _load(paths, normalize=False)
    assert ok.all()
    for row, (name, x, bps, _) in zip(out, cases):
        ref = (np.asarray(x, np.float64) * 2.0 ** -(bps - 1)).astype(np.float32)
        assert np.array_equal(row[:len(ref)], ref), name
        assert not row[len(ref):].any(), name


@pytest.mark.parametrize("rate", [8000, 16000, 22050, 44100, 48000])
def test_flac_rows_equal_the_wav_rows_of_the_same_integers(dev, tmp_path, rate):
    """Every channel count 1..8 and stereo mode at this rate, bps 8/12/16/20/24 (u8 / s16 / s24 WAV, 12 and 20 bits shifted in): resample,
    mono mix, normalisation and the seeded random crop of the longer files are K0's, and the rows are bitwise equal."""
    flac, wav = [], []
    k = 0
    for ch in range(1, 9):
        modes = list(flacenc.STEREO) if ch == 2 else ["independent"]
        for mode in modes:
            bps = (8, 12, 16, 20, 24)[k % 5]
            n = int(rate * (0.6 if k % 2 else 1.7))                      # the 1.7 s files are cropped (same draw for both)
            x = flacenc.signal(n, ch, bps, seed=100 + k)
            flac.append(_write(tmp_path, f"{k}.flac", flacenc.encode(x, rate, bps, stereo=mode, blocksize=(4096, 1152, 4608)[k % 3])))
            wav.append(_write(tmp_path, f"{k}.wav", flacenc.wav_bytes(x, rate, bps)))
            k += 1
    for normalize in (False, True):
        a, oka = _load(flac, normalize, seed=rate)
        b, okb = _load(wav, normalize, seed=rate)
        assert oka.all() and okb.all() and np.array_equal(a, b)
        assert np.abs(a).max() > 0


def _mixed_dirs(tmp_path, n_files=8):
    """The same clips as an all-WAV set and as a mixed WAV / FLAC set (some 1.5 s: cropped)."""
    wavs, mixed = [], []
    for i in range(n_files):
        rate = (16000, 44100, 48000, 22050)[i % 4]
        n = int(rate * (1.5 if i % 3 == 0 else 0.8))
        x = flacenc.signal(n, 1 + i % 2, 16, seed=300 + i)
        w = _write(tmp_path, f"c{i}.wav", flacenc.wav_bytes(x, rate, 16))
        wavs.append(w)
        mixed.append(_write(tmp_path, f"c{i}.flac", flacenc.encode(x, rate, 16, stereo="mid_side" if x.shape[1] == 2 else "independent"))
                     if i % 2 == 0 else w)
    return wavs, mixed


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def test_mixed_directory_through_the_dataset_matches_the_wav_directory(dev, tmp_path):
    wavs, mixed = _mixed_dirs(tmp_path)
    proc = pkg.AudioProcessor()
    results = {}
    for name, paths in (("wav", wavs), ("mixed", mixed)):
        ds = pkg.WakewordDataset(paths[:4], paths[4:], proc, augment=False, verbose=False)
        _seed(7)
        eval_mels = torch.cat([d for d, _ in pkg.DataLoader(ds, batch_size=3, shuffle=False)]).cpu().numpy()
        _seed(7)
        items = np.stack([ds[i][0].numpy() for i in range(len(ds))])
        dsa = pkg.WakewordDataset(paths[:4], paths[4:], proc, augment=True, verbose=False)
        _seed(8)
        aug_mels = torch.cat([d for d, _ in dsa.loader(batch_size=4, shuffle=True)]).cpu().numpy()
        results[name] = (eval_mels, items, aug_mels, ds.unreadable + dsa.unreadable)
    for a, b in zip(results["wav"], results["mixed"]):
        assert np.array_equal(a, b)
    assert results["mixed"][3] == 0 and np.abs(results["mixed"][0]).max() > 0


@pytest.mark.parametrize("duration", [0.5, 1.0, 2.0])
def test_predict_wakeword_on_flac_equals_wav(dev, tmp_path, duration):
    cfg = type(f"AudioConfig{duration}", (AudioConfig,), {"DURATION": duration})
    sd = pkg.synth.make_state_dict("simple", seed=1234)
    m = pkg.SimpleWakewordModel(audio_config=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(dev).eval()
    proc = pkg.AudioProcessor(cfg)
    x = flacenc.signal(int(44100 * 2.6), 2, 24, seed=9)                 # longer than every duration: a random crop
    w = _write(tmp_path, "p.wav", flacenc.wav_bytes(x, 44100, 24))
    f = _write(tmp_path, "p.flac", flacenc.encode(x, 44100, 24, stereo="left_side"))
    got = []
    for p in (w, f):
        random.seed(3)
        got.append(pkg.predict_wakeword(p, m, proc, dev, threshold=0.5))
        random.seed(3)
        got.append(proc.process_audio_file(p))
    assert got[0] == got[2] and got[0][1] > 0.0
    assert np.array_equal(np.asarray(got[1]), np.asarray(got[3]))


def _inconsistent(x):
    """One-frame files whose CRCs verify but whose bitstream does not hold together."""
    out = []
    data = bytearray(flacenc.encode(x[:4096], 16000, 16, subframe="verbatim", blocksize=4096))
    ff = flacenc.first_frame_offset(bytes(data))
    assert data[ff + 6] >> 1 == 0b0000001                  # header of 6 bytes, then the subframe: pad, type 000001 (VERBATIM), wasted
    bad = bytearray(data)
    bad[ff + 6] = (bad[ff + 6] & 1) | (0b000010 << 1)      # a reserved subframe type
    bad[-2:] = flacenc.crc16(bytes(bad[ff:-2])).to_bytes(2, "big")
    out.append(bytes(bad))
    cut = bytearray(data[:-300])                           # subframes that run past the end of the frame
    cut[-2:] = flacenc.crc16(bytes(cut[ff:-2])).to_bytes(2, "big")
    out.append(bytes(cut))
    return out


def test_damaged_files_give_zero_rows_and_leave_the_others_alone(dev, tmp_path):
    good = []
    for i in range(6):
        x = flacenc.signal(14000 + 500 * i, 1 + i % 2, 16, seed=500 + i)
        mode = "side_right" if x.shape[1] == 2 else "independent"
        good.append(_write(tmp_path, f"g{i}.flac", flacenc.encode(x, 16000, 16, stereo=mode)) if i % 2 == 0
                    else _write(tmp_path, f"g{i}.wav", flacenc.wav_bytes(x, 16000, 16)))
    src = flacenc.encode(flacenc.signal(9000, 1, 16, seed=9), 16000, 16, blocksize=1152)
    ff = flacenc.first_frame_offset(src)
    crc_bad = bytearray(src)
    crc_bad[ff + 300] ^= 0x04
    damaged = [_write(tmp_path, "crc.flac", bytes(crc_bad)), _write(tmp_path, "cut.flac", src[:-5])]
    inconsistent = [_write(tmp_path, f"inc{i}.flac", d) for i, d in enumerate(_inconsistent(flacenc.signal(4096, 1, 16, seed=2)[:, 0]))]
    ref, ok_ref = _load(good)
    batch = good[:2] + damaged[:1] + good[2:4] + inconsistent + good[4:] + damaged[1:]
    before = files.flac_errors()
    out, ok = _load(batch)
    assert files.flac_errors() - before == len(inconsistent)
    idx_good = [0, 1, 3, 4, 7, 8]
    assert np.array_equal(out[idx_good], ref) and ok_ref.all()
    assert ok.tolist() == [True, True, False, True, True, True, True, True, True, False]
    for i in (2, 5, 6, 9):
        assert not out[i].any()


def test_long_48k_stereo_file_among_one_second_files_and_repeatability(dev, tmp_path):
    rng = np.random.default_rng(0)
    t = np.arange(48000 * 60) / 48000.0
    base = 0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.1 * np.sin(2 * np.pi * 3000.0 * t)
    long_x = np.stack([np.round((base + 0.002 * rng.standard_normal(t.size)) * 32767),
                       np.round((0.8 * base + 0.002 * rng.standard_normal(t.size)) * 32767)], axis=1).astype(np.int64)
    long_x[12345] = (32767, -32768)
    flac, wav = [], []
    for i in range(7):
        x = long_x if i == 3 else flacenc.signal(16000, 1, 16, seed=700 + i)
        rate = 48000 if i == 3 else 16000
        flac.append(_write(tmp_path, f"l{i}.flac", flacenc.encode(x, rate, 16, stereo="mid_side" if i == 3 else "independent")))
        wav.append(_write(tmp_path, f"l{i}.wav", flacenc.wav_bytes(x, rate, 16)))
    a1, ok1 = _load(flac, seed=4)
    a2, ok2 = _load(flac, seed=4)
    b, okb = _load(wav, seed=4)
    assert ok1.all() and ok2.all() and okb.all()
    assert np.array_equal(a1, a2) and np.array_equal(a1, b)
    # the stream() path: the same rows
    rd = WavBatchReader(max_clips=4, max_raw_bytes=64 << 20, slots=3)
    random.seed(4)
    rows = np.concatenate([o.cpu().numpy() for o, _ in rd.stream(flac, 4, verbose=False)])
    rd.close()
    random.seed(4)
    rd = WavBatchReader(max_clips=4, max_raw_bytes=64 << 20, slots=3)
    rows_w = np.concatenate([o.cpu().numpy() for o, _ in rd.stream(wav, 4, verbose=False)])
    rd.close()
    assert np.array_equal(rows, rows_w)


def test_load_audio_and_process_audio_file_on_flac_equal_wav(dev, tmp_path):
    """AudioProcessor.load_audio (the whole file at 16 kHz, one K0 launch over its 1 s windows) and process_audio_file on FLAC equal the
    WAV of the same integers bit for bit -- short and long files, resampled and not, mono and stereo."""
    proc = pkg.AudioProcessor()
    cases = [(16000, 0.7, 1, 16, "independent"), (48000, 2.6, 2, 16, "mid_side"), (44100, 1.3, 2, 24, "left_side"),
             (16000, 3.2, 1, 12, "independent"), (22050, 1.0, 2, 8, "side_right")]
    for k, (rate, secs, ch, bps, mode) in enumerate(cases):
        x = flacenc.signal(int(rate * secs), ch, bps, seed=900 + k)
        w = _write(tmp_path, f"a{k}.wav", flacenc.wav_bytes(x, rate, bps))
        f = _write(tmp_path, f"a{k}.flac", flacenc.encode(x, rate, bps, stereo=mode, blocksize=(4096, 1152)[k % 2]))
        aw, af = proc.load_audio(w), proc.load_audio(f)
        assert af is not None and af.dtype == np.float32 and len(af) == len(aw) and np.array_equal(af, aw), (rate, secs, ch)
        if rate == 16000 and ch == 1:
            ref = (x[:, 0].astype(np.float64) * 2.0 ** -(bps - 1)).astype(np.float32)
            assert np.array_equal(af, ref)
        for p in (w, f):
            random.seed(k)
            if p == w:
                mw = proc.process_audio_file(p)
            else:
                mf = proc.process_audio_file(p)
        assert np.array_equal(np.asarray(mw), np.asarray(mf))
    # a damaged FLAC file: the reference's print and None
    src = flacenc.encode(flacenc.signal(9000, 1, 16, seed=1), 16000, 16)
    assert proc.load_audio(_write(tmp_path, "cut.flac", src[:-9])) is None


def test_k0_on_undecoded_flac_descriptors_writes_zero_rows_and_read_descriptors_stay(dev, tmp_path):
    """K0 given a descriptor that still says WW_FMT_FLAC (the compressed frames, not samples) writes a zero row and reads nothing; a
    batch decode leaves the descriptors read() returned as they were (WW_FMT_FLAC at the staging offset)."""
    import ctypes as C
    from wakeword_jupyterlab_amd import _native as nat
    from wakeword_jupyterlab_amd.files import DESC_DTYPE
    x1 = flacenc.signal(16000, 2, 16, seed=11)
    x2 = flacenc.signal(40000, 1, 16, seed=12)
    paths = [_write(tmp_path, "k1.flac", flacenc.encode(x1, 48000, 16)), _write(tmp_path, "k2.wav", flacenc.wav_bytes(x2, 16000, 16)),
             _write(tmp_path, "k3.flac", flacenc.encode(x2, 16000, 16))]
    rd = WavBatchReader(max_clips=4)
    descs, status = rd.read(paths, 0)
    assert (status == 1).all() and descs["format"].tolist() == [nat.FMT_FLAC, nat.FMT_S16, nat.FMT_FLAC]
    before = np.array(descs, copy=True)
    raw_dev = torch.from_numpy(rd.staging(0)).to(dev)
    descs_dev = torch.from_numpy(before.view(np.uint8).reshape(3, DESC_DTYPE.itemsize)).to(dev)
    out = torch.full((3, 16000), 7.0, device=dev)
    nat.check(nat.lib.ww_decode_resample(C.c_void_p(raw_dev.data_ptr()), C.c_void_p(descs_dev.data_ptr()), 3, 1, C.c_void_p(out.data_ptr()),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    o = out.cpu().numpy()
    assert not o[0].any() and not o[2].any() and np.abs(o[1]).max() > 0
    rows = rd.decode(0, normalize=False).cpu().numpy()
    assert np.array_equal(np.asarray(descs), before)                       # decode() did not rewrite what read() returned
    assert np.array_equal(rows[2], (x2[:16000, 0] * 2.0 ** -15).astype(np.float32))
    assert np.abs(rows[0]).max() > 0
    rd.close()
