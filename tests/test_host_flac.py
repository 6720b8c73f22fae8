"""FLAC on the host side of the native reader (no GPU): the container walk (ID3v2, metadata blocks, STREAMINFO), the frame index that
gives n_frames, the refusals (32-bit, bad magic, missing STREAMINFO, CRC-8 and CRC-16 failures, a truncated last frame), and the
staging rules (the frames and their index in staging, WW_ENOSPACE sized by the decoded samples, regrow).  Files come from tests/flacenc.py."""
import ctypes as C
import os

import numpy as np
import pytest

import flacenc
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import files
from wakeword_jupyterlab_amd.files import WavBatchReader

EOPEN, ENOTRIFF, ECHUNK, EFORMAT = -1, -2, -3, -4


def _write(tmp_path, name, data):
    p = os.path.join(tmp_path, name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def _probe_status(path):
    d = nat.ClipDesc()
    return nat.lib.ww_wav_probe_host(os.fsencode(path), C.byref(d)), d


def test_format_code_and_status_text():
    assert nat.FMT_FLAC == 7
    assert "FLAC" in nat.WAV_STATUS[ENOTRIFF]


@pytest.mark.parametrize("case", ["plain", "metadata", "id3", "total0_variable", "explicit", "stereo48k"])
def test_probe_reads_streaminfo_and_counts_frames_from_the_index(tmp_path, case):
    n, ch, rate, kw = 21000, 1, 16000, {}
    if case == "metadata":
        kw = dict(metadata=[(1, bytes(4000)), (4, b"\x03\0\0\0abc\0\0\0\0"), (6, bytes(90000)), (2, b"appl" + bytes(9)), (77, b"unknown")])
    elif case == "id3":
        kw = dict(id3=500, metadata=[(1, bytes(10))])
    elif case == "total0_variable":
        kw = dict(total_samples_zero=True, variable=[4096, 192, 16000, 712])
    elif case == "explicit":
        kw = dict(blocksize=1000, explicit_rate=True, explicit_blocksize=True, bps_from_streaminfo=True)
        rate = 12345
    elif case == "stereo48k":
        n, ch, rate, kw = 50000, 2, 48000, dict(stereo="mid_side")
    data = flacenc.encode(flacenc.signal(n, ch, 16, seed=3), rate, 16, **kw)
    p = _write(tmp_path, "a.flac", data)
    info = files.probe(p)
    assert info is not None
    assert info["format"] == nat.FMT_FLAC and info["n_frames"] == n and info["channels"] == ch and info["sample_rate"] == rate
    assert info["data_offset"] == flacenc.first_frame_offset(data)
    if rate == 48000:
        assert (info["up"], info["down"]) == (1, 3)


def test_refusals(tmp_path):
    good = flacenc.encode(flacenc.signal(9000, 1, 16, seed=4), 16000, 16, blocksize=1152)
    ff = flacenc.first_frame_offset(good)
    cases = {}
    cases["bits32"] = (flacenc.encode(np.arange(-500, 500) * 1000003, 16000, 32, subframe="verbatim"), EFORMAT)
    cases["magic"] = (b"fLaX" + good[4:], ENOTRIFF)
    cases["no_streaminfo"] = (b"fLaC" + flacenc.metadata_block(1, bytes(34), last=True) + good[ff:], ECHUNK)
    streaminfo_not_first = b"fLaC" + flacenc.metadata_block(1, bytes(8)) + bytes([0x80]) + good[5:ff] + good[ff:]
    cases["streaminfo_second"] = (streaminfo_not_first, ECHUNK)
    hdr = bytearray(good)
    hdr[ff + 4] ^= 0x01                                    # the first frame number: CRC-8 fails
    cases["crc8"] = (bytes(hdr), ECHUNK)
    cases["truncated"] = (good[:-7], ECHUNK)
    body = bytearray(good)
    body[ff + 400] ^= 0x10                                 # a bit inside the first frame: CRC-16 fails
    cases["crc16"] = (bytes(body), ECHUNK)
    cases["no_frames"] = (good[:ff], ECHUNK)
    cases["junk_mp3"] = (b"not audio", ENOTRIFF)
    cases["id3_mp3"] = (flacenc.id3v2(200) + b"\xff\xfb\x90\x64" + bytes(400), ENOTRIFF)
    cases["riff_junk"] = (b"RIFF....WAVEjunk", ECHUNK)
    paths = []
    for name, (data, want) in cases.items():
        p = _write(tmp_path, name + ".flac", data)
        st, _ = _probe_status(p)
        assert st == want, name
        paths.append(p)
    paths.append(_write(tmp_path, "good.flac", good))
    rd = WavBatchReader(max_clips=32, host_only=True, threads=3)
    descs, status = rd.read(paths, 0)
    assert list(status[:-1]) == [w for _, w in cases.values()]
    assert status[-1] == 1 and descs["n_frames"][-1] == 9000 and descs["format"][-1] == nat.FMT_FLAC
    assert (descs["n_frames"][:-1] == 0).all()
    rd.close()


def test_staging_holds_the_frames_and_their_index(tmp_path):
    a = flacenc.encode(flacenc.signal(16000, 1, 16, seed=5), 16000, 16)
    b = flacenc.encode(flacenc.signal(20000, 2, 24, seed=6), 44100, 24, stereo="left_side", blocksize=4608, id3=64)
    # a file longer than the reader's 68 KB head window: read straight into staging, then indexed there
    c = flacenc.encode(flacenc.signal(90000, 2, 16, seed=7), 22050, 16, subframe="verbatim")
    w = flacenc.wav_bytes(flacenc.signal(1000, 1, 16), 16000, 16)
    paths = [_write(tmp_path, n, d) for n, d in (("a.flac", a), ("b.flac", b), ("c.flac", c), ("w.wav", w))]
    rd = WavBatchReader(max_clips=8, max_raw_bytes=4 << 20, host_only=True, threads=2)
    descs, status = rd.read(paths, 0)
    assert (status == 1).all()
    st = rd.staging(0)
    for d, data, n, ch, rate in zip(descs[:3], (a, b, c), (16000, 20000, 90000), (1, 2, 2), (16000, 44100, 22050)):
        ff = flacenc.first_frame_offset(data)
        assert (d["format"], d["n_frames"], d["channels"], d["sample_rate"]) == (nat.FMT_FLAC, n, ch, rate)
        off = int(d["byte_offset"])
        assert off % 16 == 0 and bytes(st[off:off + len(data) - ff]) == data[ff:]
    assert descs["format"][3] == nat.FMT_S16 and descs["n_frames"][3] == 1000
    rd.close()


def test_enospace_counts_the_decoded_samples_and_regrow_fits(tmp_path):
    """Compressed bytes and decoded float32 samples are each held to the reader's capacity: a batch of highly compressible files needs
    far more for its samples than for its bytes, and WW_ENOSPACE reports that larger size."""
    data = flacenc.encode(np.zeros(48000, np.int64), 16000, 16)          # CONSTANT subframes: tens of bytes for 3 s
    assert len(data) < 200
    paths = [_write(tmp_path, f"z{i}.flac", data) for i in range(6)]
    rd = WavBatchReader(max_clips=8, max_raw_bytes=1 << 16, host_only=True, threads=2)
    with pytest.raises(nat.NativeError) as e:
        rd.read(paths, 0)
    assert e.value.code == nat.WW_ENOSPACE and e.value.needed >= 6 * 48000 * 4
    rd.regrow(8, e.value.needed)
    descs, status = rd.read(paths, 0)
    assert (status == 1).all() and (descs["n_frames"] == 48000).all()
    rd.close()


def test_enospace_of_a_file_beyond_the_head_window_reports_its_decoded_size(tmp_path):
    """A file larger than the reader's head window that does not fit the staging is still indexed (aside), so that one regrow to the
    reported size fits the whole batch -- compressed bytes and decoded samples alike."""
    x = flacenc.signal(150000, 2, 16, seed=8)
    big = flacenc.encode(x, 48000, 16, stereo="mid_side")
    assert len(big) > 70000
    paths = [_write(tmp_path, "big.flac", big), _write(tmp_path, "s.flac", flacenc.encode(x[:3000], 48000, 16))]
    rd = WavBatchReader(max_clips=4, max_raw_bytes=1 << 16, host_only=True, threads=1)
    with pytest.raises(nat.NativeError) as e:
        rd.read(paths, 0)
    assert e.value.needed >= (150000 + 3000) * 2 * 4
    rd.regrow(4, e.value.needed)
    descs, status = rd.read(paths, 0)
    assert (status == 1).all() and descs["n_frames"].tolist() == [150000, 3000]
    rd.close()


def test_stream_and_load_paths_on_a_host_reader(tmp_path):
    """stream() over FLAC and WAV files on a host-only reader: every batch's status comes from the host."""
    paths = []
    for i in range(10):
        x = flacenc.signal(8000 + 100 * i, 1, 16, seed=i)
        if i % 3:
            paths.append(_write(tmp_path, f"f{i}.flac", flacenc.encode(x, 16000, 16, blocksize=2048)))
        else:
            paths.append(_write(tmp_path, f"w{i}.wav", flacenc.wav_bytes(x, 16000, 16)))
    paths.append(_write(tmp_path, "bad.flac", b"fLaC" + bytes(50)))
    rd = WavBatchReader(max_clips=4, max_raw_bytes=1 << 20, slots=3, host_only=True, threads=2)
    oks = [ok for _, ok in rd.stream(paths, 4, verbose=False)]
    assert np.concatenate(oks).tolist() == [True] * 10 + [False]
    rd.close()
