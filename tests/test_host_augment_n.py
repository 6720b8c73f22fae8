"""Augmentation at clip lengths of 4,000 .. 16,383 samples, host side (no GPU): the records ww_augment_plans_prepare_n writes against
librosa's length arithmetic (Python's round / ceil), the refusals of the *_n entry points, and the AudioProcessor bounds."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd.config import AudioConfig

NS = (4000, 5001, 8000, 12345, 15872, 16000, 16383)
# the per-clip record of csrc/ww_augment.hip (AugDev); its size is the ABI's ww_augment_record_bytes()
REC = np.dtype([("shift", "<i4"), ("crop", "<i4"), ("p_out", "<i4"), ("p_len", "<i4"), ("p_res", "<i4"), ("s_out", "<i4"),
                ("s_len", "<i4"), ("seed", "<u4"), ("p_rate", "<f8"), ("p_ratio", "<f8"), ("s_rate", "<f8"), ("sigma", "<f4"),
                ("pad", "<f4")])


def _cfg(duration):
    return type("Cfg", (AudioConfig,), {"DURATION": duration})


def _plans(plans):
    arr = (nat.AugmentPlan * max(1, len(plans)))()
    for a, p in zip(arr, plans):
        a.shift, a.crop_start = p.get("shift", 0), p.get("crop", 0)
        a.pitch_rate = p.get("pitch_rate", 0.0)
        a.stretch_rate = p.get("rate", 0.0)
        a.noise_sigma, a.noise_seed = p.get("sigma", 0.0), p.get("seed", 0)
    return arr


def _prepare(plans, n):
    rec = np.zeros(max(1, len(plans)), dtype=REC)
    rc = nat.lib.ww_augment_plans_prepare_n(C.cast(_plans(plans), C.c_void_p), len(plans), n, C.c_void_p(rec.ctypes.data))
    return rc, rec[:len(plans)]


def _code(plans, n):
    rc, _ = _prepare(plans, n)
    return rc


def test_record_size_is_unchanged():
    assert nat.lib.ww_augment_record_bytes() == REC.itemsize == 64


@pytest.mark.parametrize("n", NS)
def test_record_lengths_follow_python_round_and_ceil(n):
    T = 1 + n // 512
    rng = random.Random(n)
    rates = [32 / 46 + 1e-9, 0.7, 0.7071, 0.8409, 1.0, 1.1892, 1.3, 1.4142, T - 0.01]
    rates += [rng.uniform(0.7, 1.3) for _ in range(40)]
    plans = []
    for r in rates:
        s_len = round(n / r)
        plans.append({"shift": rng.randint(-40000, 40000), "pitch_rate": r, "rate": r, "crop": rng.randint(0, max(0, s_len - n)),
                      "sigma": 0.15, "seed": rng.getrandbits(32)})
    rc, rec = _prepare(plans, n)
    assert rc == nat.WW_OK, nat.lib.ww_last_error()
    for p, d in zip(plans, rec):
        r = p["rate"]
        assert d["shift"] == p["shift"] % n                       # np.roll: the shift mod N, in [0, N)
        assert d["p_out"] == d["s_out"] == math.ceil(T / r)        # len(np.arange(0, T, rate))
        assert d["p_len"] == d["s_len"] == round(n / r)            # time_stretch's length: Python round(), half to even
        ratio = 16000.0 / (16000.0 / r)
        assert d["p_ratio"] == ratio and d["p_res"] == math.ceil(d["p_len"] * ratio)
        assert d["crop"] == p["crop"] <= max(0, d["s_len"] - n)
        assert d["p_rate"] == d["s_rate"] == r and d["seed"] == p["seed"] and d["sigma"] == np.float32(0.15)
    # off stages leave their fields zero
    rc, rec = _prepare([{"shift": -1}], n)
    assert rc == nat.WW_OK and rec[0]["shift"] == n - 1 and rec[0]["p_out"] == rec[0]["s_out"] == 0


def test_records_at_16000_equal_the_one_second_call():
    rng = random.Random(5)
    from oracle import augment_oracle as ao
    plans = []
    for _ in range(64):
        p = ao.draw_plan(rng)
        plans.append({"shift": p["shift"], "crop": p["crop"], "rate": p["rate"] or 0.0, "sigma": p["sigma"], "seed": p["seed"],
                      "pitch_rate": ao.pitch_rate(p["n_steps"]) if p["n_steps"] is not None else 0.0})
    rc, rec_n = _prepare(plans, 16000)
    rec = np.zeros(len(plans), dtype=REC)
    assert rc == nat.WW_OK
    assert nat.lib.ww_augment_plans_prepare(C.cast(_plans(plans), C.c_void_p), len(plans), C.c_void_p(rec.ctypes.data)) == nat.WW_OK
    assert rec.tobytes() == rec_n.tobytes()


def test_n_samples_outside_the_range_is_refused_before_any_launch():
    dummy = C.c_void_p(1 << 20)                                    # never dereferenced: the checks come first
    plans = _plans([{}])
    for n in (0, -1, 3999, 16384, 16400, 32000):
        assert _code([{}], n) == nat.WW_EINVAL
        assert nat.lib.ww_augment_n_workspace_bytes(4, n) == nat.WW_EINVAL
        assert nat.lib.ww_augment_n_f32(dummy, 1, n, n, plans, dummy, n, dummy, None) == nat.WW_EINVAL
        assert nat.lib.ww_augment_records_n_f32(dummy, 1, n, n, dummy, dummy, n, dummy, None) == nat.WW_EINVAL
    for n in (4000, 16383):
        assert nat.lib.ww_augment_n_workspace_bytes(4, n) > 0
    # the 1 s workspace is the N = 16000 one; shorter clips need no more
    assert nat.lib.ww_augment_n_workspace_bytes(7, 16000) == nat.lib.ww_augment_workspace_bytes(7)
    assert nat.lib.ww_augment_n_workspace_bytes(7, 5001) < nat.lib.ww_augment_workspace_bytes(7)


def test_a_bad_plan_is_refused_before_the_device_check():
    """The plain calls prepare their records before they look for a GPU, as the background and reverb calls do: a negative noise_sigma
    is WW_EINVAL on a machine without one, not WW_ENODEVICE."""
    dummy = C.c_void_p(1 << 20)                                    # never dereferenced: the checks come first
    plans = _plans([{}, {"sigma": -1.0}])
    assert nat.lib.ww_augment_f32(dummy, 2, 16000, plans, dummy, dummy, None) == nat.WW_EINVAL
    assert "plan 1: noise_sigma" in nat.lib.ww_last_error().decode()
    for n in (4000, 16000, 16383):
        assert nat.lib.ww_augment_n_f32(dummy, 2, (n + 3) & ~3, n, plans, dummy, n, dummy, None) == nat.WW_EINVAL
        assert "plan 1: noise_sigma" in nat.lib.ww_last_error().decode()


@pytest.mark.parametrize("n", NS)
def test_rates_keep_the_one_second_bounds_at_every_length(n):
    T = 1 + n // 512
    for key in ("pitch_rate", "rate"):
        assert _code([{key: 0.69}], n) == nat.WW_EUNSUPPORTED      # ceil(32 / rate) = 47 > 46 output steps
        assert _code([{key: 0.5}], n) == nat.WW_EUNSUPPORTED
        assert _code([{key: -1.0}], n) == nat.WW_EUNSUPPORTED
        assert _code([{key: float("nan")}], n) == nat.WW_EUNSUPPORTED
        assert _code([{key: float(T)}], n) == nat.WW_EUNSUPPORTED  # a single output step
        assert f"{n} samples" in nat.lib.ww_last_error().decode()
        assert _code([{key: 0.7}], n) == nat.WW_OK
        assert _code([{key: T - 0.5}], n) == nat.WW_OK
    assert _code([{"sigma": -1.0}], n) == nat.WW_EINVAL


@pytest.mark.parametrize("n", NS)
def test_crop_beyond_the_stretched_length_is_refused(n):
    for rate in (0.7, 0.83, 0.97):
        over = round(n / rate) - n
        assert _code([{"rate": rate, "crop": over}], n) == nat.WW_OK
        assert _code([{"rate": rate, "crop": over + 1}], n) == nat.WW_EINVAL
        assert str(n) in nat.lib.ww_last_error().decode()
        assert _code([{"rate": rate, "crop": -1}], n) == nat.WW_EINVAL
    assert _code([{"rate": 1.2, "crop": 1}], n) == nat.WW_EINVAL    # shorter than N: zero-padded, nothing to crop


def test_audio_processor_draws_crops_against_the_clip_length():
    for dur in (0.25, 0.5, 0.75, 1.0):
        proc = pkg.AudioProcessor(_cfg(dur))
        n = int(16000 * dur)
        random.seed(11)
        plans = [proc.draw_augment_plan() for _ in range(300)]
        assert any(p["crop"] > 0 for p in plans)
        for p in plans:
            if p["rate"] is not None:
                assert 0 <= p["crop"] <= max(0, round(n / p["rate"]) - n)
        conv = [{"shift": p["shift"], "crop": p["crop"], "rate": p["rate"] or 0.0, "sigma": p["sigma"], "seed": p["seed"],
                 "pitch_rate": 2.0 ** (-p["n_steps"] / 12.0) if p["n_steps"] is not None else 0.0} for p in plans]
        assert _code(conv, n) == nat.WW_OK, nat.lib.ww_last_error()   # every draw of the reference's mix is accepted


def test_longer_clips_still_refuse_augmentation():
    proc = pkg.AudioProcessor(_cfg(1.5))
    with pytest.raises(NotImplementedError, match="augmentation"):
        proc.augment_audio(np.zeros(24000, np.float32))
    with pytest.raises(NotImplementedError, match="augmentation"):
        proc.augment_batch(np.zeros((2, 24000), np.float32))
    with pytest.raises(NotImplementedError, match="augmentation"):
        proc.process_audio_file("missing.wav", augment=True)
    with pytest.raises(NotImplementedError, match="augmentation"):
        pkg.AudioProcessor(_cfg(1.025)).augment_audio(np.zeros(16400, np.float32))   # T = 33
