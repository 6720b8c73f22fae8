"""Reverberation, host side (no GPU): the configuration default, the random draws of AudioProcessor.draw_augment_plan with and without
an RIR bank, the trimming rule, the record layout and the refusals of the reverb calls, which all come before anything is launched, and
the argument checks of ops.augment / ops.reverb."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import reverb_ref
from oracle import augment_oracle as ao
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import ops, reverb
from wakeword_jupyterlab_amd.audio import AudioProcessor
from wakeword_jupyterlab_amd.config import AudioConfig, AugmentationConfig

AUG_BYTES, BG_BYTES, RIR_BYTES = 64, 32, 16
DUMMY = C.c_void_p(1 << 20)                                   # never dereferenced: the checks come first
RIR = np.dtype([("index", "<i8"), ("dpos", "<i4"), ("pad", "<i4")])


class _FakeBank:
    def __init__(self, lengths):
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)

    @property
    def n_files(self):
        return len(self.lengths)


class _FakeRirs:
    def __init__(self, n):
        self.n_rirs = n


def _bare_processor(duration=1.0):
    proc = AudioProcessor.__new__(AudioProcessor)
    proc.config = type("Cfg", (AudioConfig,), {"DURATION": duration})
    return proc


def _rir(entries):
    arr = (nat.AugmentRir * max(1, len(entries)))()
    for a, e in zip(arr, entries):
        a.index, a.dpos, a.taps, a.enabled = e.get("index", 0), e.get("dpos", 0), e.get("taps", 1), e.get("enabled", 1)
    return arr


def _plans(n):
    return (nat.AugmentPlan * max(1, n))()


def test_config_and_abi_constants():
    assert AugmentationConfig.RIR_PROB == 0.5
    assert AugmentationConfig.BACKGROUND_PROB == 0.8 and AugmentationConfig.AUGMENTATION_PROB == 0.8     # unchanged
    assert (nat.RIR_MAX_TAPS, nat.RIR_FFT_SIZE, nat.RIR_SPECTRUM_BINS) == (16384, 32768, 16385)
    assert C.sizeof(nat.AugmentRir) == 24
    assert nat.lib.ww_augment_rir_record_bytes() == AUG_BYTES + BG_BYTES + RIR_BYTES
    assert nat.lib.ww_augment_bg_record_bytes() == AUG_BYTES + BG_BYTES and nat.lib.ww_augment_record_bytes() == AUG_BYTES
    assert nat.lib.ww_abi_version() == 4


@pytest.mark.parametrize("duration", [1.0, 0.5])
def test_without_an_rir_bank_the_stream_and_plans_are_unchanged(duration):
    """No RIR bank (or RIR_PROB = 0): the random stream, the plans and their exact keys are those of the code before reverb, with and
    without a background bank."""
    n = int(16000 * duration)
    proc = _bare_processor(duration)
    random.seed(11)
    got = [proc.draw_augment_plan() for _ in range(200)]
    rng = random.Random(11)
    assert got == [ao.draw_plan(rng, n=n) for _ in range(200)]
    assert random.random() == rng.random()
    proc._background = _FakeBank([5000, 30000])
    random.seed(12)
    with_bg = [proc.draw_augment_plan() for _ in range(200)]
    proc._rirs = _FakeRirs(7)
    off = type("Aug", (AugmentationConfig,), {"RIR_PROB": 0.0})
    random.seed(12)
    with_bg_off = [proc.draw_augment_plan(off) for _ in range(200)]
    proc._rirs = None
    random.seed(12)
    again = [proc.draw_augment_plan() for _ in range(200)]
    assert with_bg == with_bg_off == again
    assert not any("rir" in p for p in with_bg)


def test_with_an_rir_bank_the_draw_follows_the_background_draws():
    lengths = [48000, 700]
    proc = _bare_processor()
    proc._background = _FakeBank(lengths)
    proc._rirs = _FakeRirs(5)
    random.seed(99)
    got = [proc.draw_augment_plan() for _ in range(600)]
    rng = random.Random(99)
    for p in got:
        want = ao.draw_plan(rng)
        if rng.random() < AugmentationConfig.BACKGROUND_PROB:
            f = rng.randrange(len(lengths))
            want.update(bg_file=f, bg_start=rng.randrange(lengths[f]), snr_db=rng.uniform(0.0, 40.0))
        if rng.random() < AugmentationConfig.RIR_PROB:
            want["rir"] = rng.randrange(5)
        assert p == want and list(p) == list(want)
    on = sum("rir" in p for p in got) / len(got)
    assert 0.4 < on < 0.6
    assert {p["rir"] for p in got if "rir" in p} == set(range(5))
    assert random.random() == rng.random()


def test_rir_only_bank_draws():
    proc = _bare_processor(0.5)
    proc._rirs = _FakeRirs(3)
    cfg = type("Aug", (AugmentationConfig,), {"RIR_PROB": 1.0})
    random.seed(3)
    got = [proc.draw_augment_plan(cfg) for _ in range(50)]
    rng = random.Random(3)
    for p in got:
        want = ao.draw_plan(rng, n=8000)
        rng.random()
        want["rir"] = rng.randrange(3)
        assert p == want


@pytest.mark.parametrize("length,spike,want", [
    (1, 0, (0, 1, 0)),                      # one tap
    (97, 10, (0, 97, 10)),                  # direct path inside the first 40 taps: nothing cut in front
    (4000, 40, (0, 4000, 40)),
    (4000, 41, (1, 3999, 40)),
    (16384, 300, (260, 16124, 40)),
    (30000, 300, (260, 16384, 40)),         # cut to 16384 taps
    (40000, 30000, (29960, 10040, 40)),     # a late direct path: the tail after it is what remains
])
def test_trimming_rule(length, spike, want):
    h = reverb_ref.decaying_rir(length, spike, seed=length)
    assert reverb.trim_bounds(h) == want
    assert reverb.trim_bounds(torch.from_numpy(h)) == want
    kept, dpos = reverb_ref.trim(h)
    assert (kept.size, dpos) == want[1:]
    assert np.array_equal(kept, h[want[0]:want[0] + want[1]])


def test_trimming_takes_the_first_maximum():
    h = np.zeros(500, np.float32)
    h[[100, 200, 300]] = [0.5, -0.5, 0.5]
    assert reverb.trim_bounds(h) == (60, 440, 40)
    assert reverb.trim_bounds(torch.from_numpy(h)) == (60, 440, 40)


def test_prepare_writes_the_reverb_records():
    entries = [{"index": 2, "dpos": 40, "taps": 16384}, {"enabled": 0, "index": -9, "dpos": -1, "taps": 0},
               {"index": 0, "dpos": 0, "taps": 1}]
    n = len(entries)
    rec = np.zeros(n * (AUG_BYTES + BG_BYTES + RIR_BYTES), dtype=np.uint8)
    rc = nat.lib.ww_augment_rir_prepare(C.cast(_plans(n), C.c_void_p), None, C.cast(_rir(entries), C.c_void_p), n, 16000, 0, 3,
                                        C.c_void_p(rec.ctypes.data))
    assert rc == nat.WW_OK, nat.lib.ww_last_error()
    r = rec[n * (AUG_BYTES + BG_BYTES):].view(RIR)
    assert r[0]["index"] == 2 and r[0]["dpos"] == 40
    assert r[1]["index"] == -1 and r[1]["dpos"] == 0
    assert r[2]["index"] == 0 and r[2]["dpos"] == 0
    assert not rec[n * AUG_BYTES:n * (AUG_BYTES + BG_BYTES)].any()             # no background: zero records


BAD = [({"index": 3, "taps": 10}, "index"), ({"index": -1, "taps": 10}, "index"), ({"dpos": 10, "taps": 10}, "dpos"),
       ({"dpos": -1, "taps": 10}, "dpos"), ({"taps": 0}, "taps"), ({"taps": 16385, "dpos": 0}, "taps")]


@pytest.mark.parametrize("entry,word", BAD)
def test_refusals_before_any_launch(entry, word):
    """Every reverb call returns WW_EINVAL for a bad record before it touches the (bogus) device pointers."""
    n = 2
    rir = _rir([{"enabled": 0}, entry])
    rec = np.zeros(n * (AUG_BYTES + BG_BYTES + RIR_BYTES), dtype=np.uint8)
    assert nat.lib.ww_augment_rir_prepare(C.cast(_plans(n), C.c_void_p), None, C.cast(rir, C.c_void_p), n, 16000, 0, 3,
                                          C.c_void_p(rec.ctypes.data)) == nat.WW_EINVAL
    assert word in nat.lib.ww_last_error().decode()
    assert nat.lib.ww_augment_rir_f32(DUMMY, n, 16000, 16000, _plans(n), None, None, 0, rir, DUMMY, 3, DUMMY, 16000, DUMMY,
                                      None) == nat.WW_EINVAL
    assert nat.lib.ww_reverb_f32(DUMMY, n, 24000, 24000, rir, DUMMY, 3, DUMMY, 24000, DUMMY, None) == nat.WW_EINVAL


@pytest.mark.parametrize("n_samples", [3999, 16384, 32001])
def test_refusals_of_lengths(n_samples):
    rir = _rir([{"index": 0, "taps": 5}])
    if n_samples > 16383:
        assert nat.lib.ww_augment_rir_workspace_bytes(1, n_samples) == nat.WW_EINVAL
        assert nat.lib.ww_augment_rir_f32(DUMMY, 1, n_samples, n_samples, _plans(1), None, None, 0, rir, DUMMY, 1, DUMMY, n_samples,
                                          DUMMY, None) == nat.WW_EINVAL
    if not 4000 <= n_samples <= 32000:
        assert nat.lib.ww_reverb_f32(DUMMY, 1, n_samples, n_samples, rir, DUMMY, 1, DUMMY, n_samples, DUMMY, None) == nat.WW_EINVAL


def test_spectra_build_refusals():
    offs = (C.c_int64 * 2)(0, 100)
    lens = (C.c_int32 * 2)(100, 16385)                                      # one RIR too long
    assert nat.lib.ww_rir_spectra_f32(DUMMY, 1 << 20, offs, lens, 2, DUMMY, DUMMY, None) == nat.WW_EINVAL
    lens = (C.c_int32 * 2)(100, 0)                                          # an empty one
    assert nat.lib.ww_rir_spectra_f32(DUMMY, 1 << 20, offs, lens, 2, DUMMY, DUMMY, None) == nat.WW_EINVAL
    lens = (C.c_int32 * 2)(100, 50)
    assert nat.lib.ww_rir_spectra_f32(DUMMY, 149, offs, lens, 2, DUMMY, DUMMY, None) == nat.WW_EINVAL     # past the buffer
    assert nat.lib.ww_rir_spectra_workspace_bytes(3) == 256
    assert nat.lib.ww_rir_spectra_workspace_bytes(-1) == nat.WW_EINVAL
    assert nat.lib.ww_reverb_workspace_bytes(17) == 512


def test_null_and_alignment_refusals():
    rir = _rir([{"index": 0, "taps": 5}])
    assert nat.lib.ww_reverb_f32(DUMMY, 1, 8000, 8000, None, DUMMY, 1, DUMMY, 8000, DUMMY, None) == nat.WW_EINVAL     # no records
    assert nat.lib.ww_reverb_f32(DUMMY, 1, 8000, 8000, rir, None, 1, DUMMY, 8000, DUMMY, None) == nat.WW_EINVAL       # no spectra
    assert nat.lib.ww_reverb_f32(DUMMY, 1, 8000, 8000, rir, C.c_void_p((1 << 20) + 4), 1, DUMMY, 8000, DUMMY, None) == nat.WW_EINVAL
    assert nat.lib.ww_reverb_f32(DUMMY, 2, 7999, 8000, _rir([{"enabled": 0}] * 2), DUMMY, 1, DUMMY, 8000, DUMMY,
                                 None) == nat.WW_EINVAL                                                            # stride < N


def test_ops_argument_checks():
    class Bank:
        n_rirs = 1
        spectra = torch.zeros(1, 16385, 2)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.reverb(torch.zeros(2, 8000), Bank(), 0)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.augment(torch.zeros(2, 8000), [dict(rir=0)] * 2, rirs=Bank())
    with pytest.raises(ValueError, match="rir 3"):
        ops._rir_array([{"rir": 3}], Bank(), 1)
    arr = ops._rir_array([{}, {"rir": None}], Bank(), 2)
    assert arr[0].enabled == 0 and arr[1].enabled == 0


def test_bank_needs_a_gpu_or_a_file(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no GPU"):
        reverb.ImpulseResponseBank([str(tmp_path / "none.wav")])
