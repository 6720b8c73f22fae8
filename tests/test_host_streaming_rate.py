"""CPU-only checks of streaming at the microphone's own rate, sample format and channel count: the entry points exist with their
argtypes, ww_streamer_create_input refuses bad rates, formats, channel counts and hops before any HIP call, its latency D is K0's index
relation, and StreamingDetector refuses a bad input format before it touches a device."""
import ctypes as C
from math import gcd

import pytest
import torch

import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat

WW_EINVAL, WW_EUNSUPPORTED = -1, -4

# the hop table: rate -> (input frames per hop, 16 kHz samples per hop, D)
HOPS = {48000: (480, 160, 10), 44100: (441, 160, 10), 22050: (441, 320, 10), 11025: (441, 640, 14), 8000: (80, 160, 20)}


def _create(hop, rate, fmt=nat.FMT_S16, channels=1, n_samples=16000, n_conv=2, n_mics=2):
    handle = C.c_void_p()
    rc = nat.lib.ww_streamer_create_input(n_mics, hop, rate, fmt, channels, n_samples, C.c_void_p(16), n_conv, None, C.byref(handle))
    return rc, (nat.lib.ww_last_error() or b"").decode(), handle.value


def test_library_exports_the_input_format_entry_points():
    lib = C.CDLL(nat.LIB_PATH)
    for name, n_args in (("ww_streamer_create_input", 10), ("ww_streamer_step_input", 4), ("ww_streamer_latency", 1)):
        assert hasattr(lib, name)
        assert getattr(nat.lib, name).argtypes is not None and len(getattr(nat.lib, name).argtypes) == n_args
    assert nat.lib.ww_abi_version() == 4


@pytest.mark.parametrize("rate,hop", [(48000, 482), (44100, 440)])
def test_hop_that_is_not_a_whole_number_of_output_samples_is_einval(rate, hop):
    rc, msg, h = _create(hop, rate)
    assert rc == WW_EINVAL and "hop_frames" in msg and h is None


def test_output_hop_that_does_not_divide_the_window_is_einval():
    rc, msg, h = _create(441 * 3, 44100)                        # 480 samples at 16 kHz: not a divisor of 16000
    assert rc == WW_EINVAL and "hop_frames" in msg and h is None
    rc, msg, h = _create(18, 48000)                              # 6 samples: not a multiple of 4
    assert rc == WW_EINVAL and "hop_frames" in msg and h is None


@pytest.mark.parametrize("rate", [999, 400000])
def test_rate_out_of_range_is_einval(rate):
    rc, msg, h = _create(480, rate)
    assert rc == WW_EINVAL and "sample_rate" in msg and h is None


@pytest.mark.parametrize("fmt", [nat.FMT_FLAC, 0, 9])
def test_flac_and_unknown_formats_are_einval(fmt):
    rc, msg, h = _create(480, 48000, fmt=fmt)
    assert rc == WW_EINVAL and "format" in msg and h is None


@pytest.mark.parametrize("channels", [0, 9])
def test_channel_count_out_of_range_is_einval(channels):
    rc, msg, h = _create(480, 48000, channels=channels)
    assert rc == WW_EINVAL and "channels" in msg and h is None


def test_window_length_is_checked_first():
    rc, msg, h = _create(482, 999, fmt=nat.FMT_FLAC, channels=0, n_samples=3996)
    assert rc == WW_EUNSUPPORTED and "n_samples" in msg and h is None


def test_null_out_pointer_is_einval():
    assert nat.lib.ww_streamer_create_input(2, 480, 48000, nat.FMT_S16, 1, 16000, C.c_void_p(16), 2, None, None) == WW_EINVAL
    assert nat.lib.ww_streamer_latency(None) == WW_EINVAL


def test_valid_combinations_reach_the_model_check():
    fmts = (nat.FMT_S16, nat.FMT_F32, nat.FMT_S24, nat.FMT_S32, nat.FMT_U8, nat.FMT_F64)
    for rate, (hop, _, _) in HOPS.items():
        for fmt in fmts:
            for ch in (1, 2, 8):
                rc, msg, h = _create(hop, rate, fmt=fmt, channels=ch, n_conv=5)
                assert rc == WW_EINVAL and "n_conv" in msg and h is None, (rate, fmt, ch, rc, msg)
    for rate, hop, n in ((16000, 160, 16000), (16000, 80, 8000), (48000, 12, 16000), (48000, 60, 4000), (96000, 96, 16000)):
        rc, msg, h = _create(hop, rate, fmt=nat.FMT_F32, n_samples=n, n_conv=5)
        assert rc == WW_EINVAL and "n_conv" in msg and h is None, (rate, hop, n, rc, msg)


def _latency_brute_force(rate, hop_in, hops=6):
    """K0's output index relation, evaluated: after k hops of hop_in frames, which 16 kHz samples have every input frame of their
    filter?  D = k * hop_out - that count (the same for every k)."""
    g = gcd(16000, rate)
    up, down = 16000 // g, rate // g
    half_len = 10 * max(up, down)
    n_pre_pad = down - half_len % down
    n_pre_remove = (half_len + n_pre_pad) // down
    hop_out = hop_in * up // down
    lags = set()
    for k in range(1, hops + 1):
        n_in = k * hop_in
        done = 0
        while True:                                              # output j needs frames up to floor(c / up)
            c = (done + n_pre_remove) * down - n_pre_pad
            if c // up > n_in - 1:
                break
            done += 1
        lags.add(k * hop_out - done)
    assert len(lags) == 1
    return lags.pop()


@pytest.mark.parametrize("rate", sorted(HOPS))
def test_latency_is_k0s_index_relation(rate):
    hop, hop_out, d = HOPS[rate]
    up, down, hl = C.c_int32(), C.c_int32(), C.c_int32()
    nat.lib.ww_resample_taps_host(rate, None, 0, C.byref(up), C.byref(down), C.byref(hl))
    assert hop * up.value == hop_out * down.value
    assert _latency_brute_force(rate, hop) == d
    # ww_streamer_latency reads D from a handle, which needs a device: tests/test_gpu_streaming_rate.py compares it with this table


def test_detector_refuses_bad_input_formats_before_any_device():
    m = pkg.SimpleWakewordModel().eval()                         # on the CPU: passing the checks would end in "no CPU path"
    with pytest.raises(TypeError, match="dtype"):
        pkg.StreamingDetector(m, n_mics=2, dtype=torch.float64)
    with pytest.raises(TypeError, match="dtype"):
        pkg.StreamingDetector(m, n_mics=2, sample_rate=48000, hop_samples=480, dtype=torch.int32)
    for ch in (0, 9):
        with pytest.raises(ValueError, match="channels"):
            pkg.StreamingDetector(m, n_mics=2, sample_rate=48000, hop_samples=480, channels=ch)
    with pytest.raises(TypeError, match="channels"):
        pkg.StreamingDetector(m, n_mics=2, channels=2.0)
    for rate in (999, 400000):
        with pytest.raises(ValueError, match="sample_rate"):
            pkg.StreamingDetector(m, n_mics=2, sample_rate=rate)
    for rate, hop in ((48000, 482), (44100, 440), (44100, 441 * 3), (48000, 160)):
        with pytest.raises(ValueError, match="hop_samples"):
            pkg.StreamingDetector(m, n_mics=2, sample_rate=rate, hop_samples=hop, dtype=torch.int16)
    for rate, (hop, _, _) in HOPS.items():                      # valid: refused only for the missing device
        with pytest.raises(RuntimeError, match="no CPU path"):
            pkg.StreamingDetector(m, n_mics=2, sample_rate=rate, hop_samples=hop, channels=2, dtype=torch.int16)
