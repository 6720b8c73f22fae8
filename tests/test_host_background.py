"""Background noise, host side (no GPU): the configuration defaults, the random draws of AudioProcessor.draw_augment_plan with and
without a bank, the records ww_augment_bg_prepare writes (int64 offsets, wrap-around starts) and the refusals of the background calls,
which all come before anything is launched."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import wakeword_jupyterlab_amd as pkg
from oracle import augment_oracle as ao
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd.audio import AudioProcessor
from wakeword_jupyterlab_amd.config import AudioConfig, AugmentationConfig

# the records of csrc/ww_augment.hip: [n] AugDev (64 bytes) then [n] BgDev
BG = np.dtype([("off", "<i8"), ("len", "<i8"), ("start", "<i8"), ("snr_lin", "<f8")])
AUG_BYTES = 64
DUMMY = C.c_void_p(1 << 20)                                   # never dereferenced: the checks come first


class _FakeBank:
    """What draw_augment_plan reads of a bank: the file count and lengths."""

    def __init__(self, lengths):
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)

    @property
    def n_files(self):
        return len(self.lengths)


def _bare_processor(duration=1.0):
    proc = AudioProcessor.__new__(AudioProcessor)             # no __init__, as tests/test_oracle_augment.py builds it
    proc.config = type("Cfg", (AudioConfig,), {"DURATION": duration})
    return proc


def _bg(entries):
    arr = (nat.AugmentBg * max(1, len(entries)))()
    for a, e in zip(arr, entries):
        a.file_offset, a.file_len, a.start = e.get("off", 0), e.get("len", 0), e.get("start", 0)
        a.snr_db, a.enabled = e.get("snr", 0.0), e.get("enabled", 1)
    return arr


def _plans(n):
    return (nat.AugmentPlan * max(1, n))()


def _prepare(entries, n_samples=16000, bank_len=1 << 20):
    n = len(entries)
    rec = np.zeros(n * (AUG_BYTES + BG.itemsize), dtype=np.uint8)
    rc = nat.lib.ww_augment_bg_prepare(C.cast(_plans(n), C.c_void_p), C.cast(_bg(entries), C.c_void_p), n, n_samples, bank_len,
                                       C.c_void_p(rec.ctypes.data))
    return rc, rec[n * AUG_BYTES:].view(BG)


def test_config_defaults():
    assert AugmentationConfig.BACKGROUND_PROB == 0.8
    assert AugmentationConfig.BACKGROUND_SNR_MIN == 0.0 and AugmentationConfig.BACKGROUND_SNR_MAX == 40.0
    assert AugmentationConfig.AUGMENTATION_PROB == 0.8 and AugmentationConfig.NOISE_FACTOR == 0.15       # the reference's, unchanged


def test_record_size():
    assert nat.lib.ww_augment_bg_record_bytes() == AUG_BYTES + BG.itemsize == 96
    assert C.sizeof(nat.AugmentBg) == 32
    assert nat.lib.ww_augment_record_bytes() == AUG_BYTES                  # the existing record is unchanged


@pytest.mark.parametrize("duration", [1.0, 0.5, 0.25])
def test_without_a_bank_the_draws_are_the_reference_ones(duration):
    n = int(16000 * duration)
    proc = _bare_processor(duration)
    random.seed(321)
    got = [proc.draw_augment_plan() for _ in range(200)]
    rng = random.Random(321)
    assert got == [ao.draw_plan(rng, n=n) for _ in range(200)]
    assert random.random() == rng.random()                                 # the stream is left where the oracle leaves it
    # a detached bank, or BACKGROUND_PROB = 0, draws nothing either
    proc._background = None
    random.seed(5)
    a = [proc.draw_augment_plan() for _ in range(50)]
    proc._background = _FakeBank([1000, 20])
    off = type("Aug", (AugmentationConfig,), {"BACKGROUND_PROB": 0.0})
    random.seed(5)
    b = [proc.draw_augment_plan(off) for _ in range(50)]
    rng = random.Random(5)
    assert a == b == [ao.draw_plan(rng, n=n) for _ in range(50)]


def test_with_a_bank_the_extra_draws_follow_the_reference_ones():
    lengths = [48000, 700, 2 ** 31 + 12345, 1]
    proc = _bare_processor()
    proc._background = _FakeBank(lengths)
    random.seed(77)
    got = [proc.draw_augment_plan() for _ in range(400)]
    rng = random.Random(77)
    for p in got:
        want = ao.draw_plan(rng)                                          # the reference's four draws (and the crop) first
        assert {k: p[k] for k in want} == want
        if rng.random() < AugmentationConfig.BACKGROUND_PROB:
            f = rng.randrange(len(lengths))
            assert p["bg_file"] == f
            assert p["bg_start"] == rng.randrange(lengths[f])
            assert p["snr_db"] == rng.uniform(0.0, 40.0)
            assert 0 <= p["bg_start"] < lengths[f] and 0.0 <= p["snr_db"] <= 40.0
        else:
            assert set(p) == set(want)                                     # no background: not even None-valued keys
    on = sum("bg_file" in p for p in got) / len(got)
    assert 0.7 < on < 0.9
    assert {p["bg_file"] for p in got if "bg_file" in p} == set(range(len(lengths)))
    assert any(p["bg_start"] >= 2 ** 30 for p in got if p.get("bg_file") == 2)          # starts drawn over the whole long file


def test_custom_snr_range_is_drawn_from():
    proc = _bare_processor()
    proc._background = _FakeBank([5000])
    cfg = type("Aug", (AugmentationConfig,), {"BACKGROUND_PROB": 1.0, "BACKGROUND_SNR_MIN": -5.0, "BACKGROUND_SNR_MAX": -4.0})
    random.seed(1)
    snrs = [proc.draw_augment_plan(cfg)["snr_db"] for _ in range(100)]
    assert all(-5.0 <= s <= -4.0 for s in snrs)


def test_records_carry_int64_offsets_and_wrapping_starts():
    big = 2 ** 31 + 1000
    entries = [{"off": big, "len": 3000, "start": 2999, "snr": 20.0},          # past 2^31, a start one sample before the wrap
               {"off": 0, "len": 7, "start": 6, "snr": -5.0},                 # a file far shorter than the clip
               {"enabled": 0, "off": -5, "len": -1, "snr": float("nan")},     # disabled: not looked at, a zero record
               {"off": big + 3000 - 1, "len": 1, "start": 0, "snr": 0.0}]     # the bank's last sample
    rc, rec = _prepare(entries, 16000, big + 3000)
    assert rc == nat.WW_OK, nat.lib.ww_last_error()
    assert rec[0]["off"] == big and rec[0]["len"] == 3000 and rec[0]["start"] == 2999
    assert math.isclose(rec[0]["snr_lin"], 100.0, rel_tol=1e-15)
    assert rec[1]["len"] == 7 and rec[1]["start"] == 6 and math.isclose(rec[1]["snr_lin"], 10 ** -0.5, rel_tol=1e-15)
    assert rec[2].tobytes() == bytes(BG.itemsize)
    assert rec[3]["off"] == big + 2999 and rec[3]["snr_lin"] == 1.0
    # the augmentation half equals ww_augment_plans_prepare_n's records
    n = 3
    plans = _plans(n)
    for i, p in enumerate(plans[:n]):
        p.shift, p.stretch_rate, p.noise_sigma, p.noise_seed = 100 * i - 7, 0.8 + 0.1 * i, 0.15, 1234 + i
    full = np.zeros(n * 96, dtype=np.uint8)
    aug = np.zeros(n * 64, dtype=np.uint8)
    assert nat.lib.ww_augment_bg_prepare(C.cast(plans, C.c_void_p), C.cast(_bg([{"enabled": 0}] * n), C.c_void_p), n, 12345, 0,
                                         C.c_void_p(full.ctypes.data)) == nat.WW_OK
    assert nat.lib.ww_augment_plans_prepare_n(C.cast(plans, C.c_void_p), n, 12345, C.c_void_p(aug.ctypes.data)) == nat.WW_OK
    assert full[:n * 64].tobytes() == aug.tobytes() and not full[n * 64:].any()


BAD = [({"off": 0, "len": 0, "start": 0}, "file_len"),
       ({"off": 0, "len": -3, "start": 0}, "file_len"),
       ({"off": -1, "len": 10, "start": 0}, "outside the bank"),
       ({"off": 995, "len": 10, "start": 0}, "outside the bank"),           # bank of 1000: the file ends past it
       ({"off": 2 ** 62, "len": 2 ** 62, "start": 0}, "outside the bank"),  # no overflow in the check
       ({"off": 0, "len": 10, "start": 10}, "start"),
       ({"off": 0, "len": 10, "start": -1}, "start"),
       ({"off": 0, "len": 10, "start": 0, "snr": float("inf")}, "snr"),
       ({"off": 0, "len": 10, "start": 0, "snr": float("-inf")}, "snr"),
       ({"off": 0, "len": 10, "start": 0, "snr": float("nan")}, "snr")]


@pytest.mark.parametrize("entry,what", BAD)
def test_every_refusal_comes_before_any_launch(entry, what):
    good = {"off": 0, "len": 1000, "start": 999, "snr": 10.0}
    bg = _bg([good, entry])
    rc, _ = _prepare([good, entry], 16000, 1000)
    assert rc == nat.WW_EINVAL and what in nat.lib.ww_last_error().decode()
    for n in (16000, 4000, 16383):
        assert nat.lib.ww_augment_bg_f32(DUMMY, 2, (n + 3) & ~3, n, _plans(2), bg, DUMMY, 1000, DUMMY, n, DUMMY, None) == nat.WW_EINVAL
        assert what in nat.lib.ww_last_error().decode()
    for n in (4000, 16000, 32000):
        assert nat.lib.ww_mix_background_f32(DUMMY, 2, n, n, bg, DUMMY, 1000, DUMMY, n, DUMMY, None) == nat.WW_EINVAL
        assert what in nat.lib.ww_last_error().decode()


def test_lengths_outside_the_range_are_refused():
    good = _bg([{"off": 0, "len": 1000, "start": 0, "snr": 10.0}])
    for n in (0, 3999, 16384, 16400, 32000):
        assert nat.lib.ww_augment_bg_workspace_bytes(2, n) == nat.WW_EINVAL
        assert nat.lib.ww_augment_bg_f32(DUMMY, 1, n, n, _plans(1), good, DUMMY, 1000, DUMMY, n, DUMMY, None) == nat.WW_EINVAL
        assert nat.lib.ww_augment_bg_records_f32(DUMMY, 1, n, n, DUMMY, DUMMY, 1000, DUMMY, n, DUMMY, None) == nat.WW_EINVAL
        assert _prepare([{"off": 0, "len": 1000, "start": 0}], n, 1000)[0] == nat.WW_EINVAL
    for n in (0, 3999, 32001, 48000):
        assert nat.lib.ww_mix_background_f32(DUMMY, 1, n, n, good, DUMMY, 1000, DUMMY, n, DUMMY, None) == nat.WW_EINVAL
    for n in (4000, 16000, 16383):
        assert nat.lib.ww_augment_bg_workspace_bytes(3, n) > nat.lib.ww_augment_n_workspace_bytes(3, n)
    assert nat.lib.ww_mix_background_workspace_bytes(3) >= 3 * BG.itemsize


def test_pointer_and_bank_refusals():
    good = _bg([{"off": 0, "len": 1000, "start": 0, "snr": 10.0}])
    # a clip that asks for background needs a bank pointer; a negative bank length is refused
    assert nat.lib.ww_augment_bg_f32(DUMMY, 1, 16000, 16000, _plans(1), good, None, 1000, DUMMY, 16000, DUMMY, None) == nat.WW_EINVAL
    assert nat.lib.ww_augment_bg_f32(DUMMY, 1, 16000, 16000, _plans(1), good, DUMMY, -1, DUMMY, 16000, DUMMY, None) == nat.WW_EINVAL
    assert nat.lib.ww_augment_bg_f32(DUMMY, 1, 16000, 16000, _plans(1), None, DUMMY, 1000, DUMMY, 16000, DUMMY, None) == nat.WW_EINVAL
    assert nat.lib.ww_mix_background_f32(DUMMY, 1, 16000, 16000, good, None, 1000, DUMMY, 16000, DUMMY, None) == nat.WW_EINVAL
    assert nat.lib.ww_augment_bg_records_f32(DUMMY, 1, 16000, 16000, DUMMY, None, 1000, DUMMY, 16000, DUMMY, None) == nat.WW_EINVAL
    # the augmentation plan is still checked (a negative sigma)
    plans = _plans(1)
    plans[0].noise_sigma = -1.0
    assert nat.lib.ww_augment_bg_f32(DUMMY, 1, 16000, 16000, plans, good, DUMMY, 1000, DUMMY, 16000, DUMMY, None) == nat.WW_EINVAL
    # nothing to do is fine without pointers
    assert nat.lib.ww_augment_bg_f32(None, 0, 16000, 16000, None, None, None, 0, None, 16000, None, None) == nat.WW_OK
    assert nat.lib.ww_mix_background_f32(None, 0, 16000, 16000, None, None, 0, None, 16000, None, None) == nat.WW_OK


def test_bank_index_from_lengths():
    bank = _FakeBank([5, 1, 7])
    assert bank.offsets.tolist() == [0, 5, 6]
    from wakeword_jupyterlab_amd.background import BackgroundNoiseBank
    b = BackgroundNoiseBank.__new__(BackgroundNoiseBank)
    b._set_index(np.array([2 ** 31, 10], dtype=np.int64))
    assert b.offsets.dtype == np.int64 and b.offsets.tolist() == [0, 2 ** 31] and b.n_samples == 2 ** 31 + 10 and b.n_files == 2


def test_background_module_and_example_flag(tmp_path):
    from wakeword_jupyterlab_amd.background import list_audio_files
    for name in ("b.wav", "a.FLAC", "c.mp3", "d.txt"):
        (tmp_path / name).write_bytes(b"")
    (tmp_path / "sub.wav").mkdir()
    assert [p.rsplit("/", 1)[1] for p in list_audio_files(str(tmp_path))] == ["a.FLAC", "b.wav"]
    assert pkg.BackgroundNoiseBank.__name__ == "BackgroundNoiseBank"
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "train_from_files.py"), "--help"], capture_output=True, text=True,
                         cwd=root, timeout=120)
    assert out.returncode == 0 and "--background" in out.stdout
