"""CPU-only checks of streaming at window lengths of 0.25 .. 1 s: the entry point exists, refuses bad lengths and hops before any HIP call,
StreamingDetector takes the model's clip length, and the deployment package records the model's own audio_config."""
import ctypes as C

import pytest
import torch

import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd.model import save_deployment_package
from wakeword_jupyterlab_amd.config import AudioConfig

WW_EINVAL, WW_EUNSUPPORTED = -1, -4


def _cfg(duration):
    return type("Cfg", (AudioConfig,), {"DURATION": duration})


def _create_n(n_mics, hop, n_samples, n_conv=2):
    handle = C.c_void_p()
    rc = nat.lib.ww_streamer_create_n(n_mics, hop, n_samples, C.c_void_p(16), n_conv, None, C.byref(handle))
    return rc, (nat.lib.ww_last_error() or b"").decode(), handle.value


def test_library_exports_streamer_create_n():
    lib = C.CDLL(nat.LIB_PATH)
    assert hasattr(lib, "ww_streamer_create_n")
    assert nat.lib.ww_streamer_create_n.argtypes is not None and len(nat.lib.ww_streamer_create_n.argtypes) == 7


@pytest.mark.parametrize("hop", [6, 170])
def test_bad_hop_at_8000_is_einval(hop):
    rc, msg, h = _create_n(2, hop, 8000)
    assert rc == WW_EINVAL and "hop_samples" in msg and h is None


def test_hop_that_does_not_divide_n_is_einval():
    rc, msg, h = _create_n(2, 160, 5000)
    assert rc == WW_EINVAL and "hop_samples 160" in msg and "5000" in msg and h is None


@pytest.mark.parametrize("hop,n", [(4, 3996), (4, 16384), (160, 20000)])
def test_length_outside_range_is_eunsupported(hop, n):
    rc, msg, h = _create_n(2, hop, n)
    assert rc == WW_EUNSUPPORTED and f"n_samples {n}" in msg and h is None


def test_length_is_checked_before_the_hop():
    rc, msg, _ = _create_n(2, 6, 3996)                    # both wrong: the length wins
    assert rc == WW_EUNSUPPORTED and "n_samples" in msg
    rc, msg, _ = _create_n(2, 170, 32000)
    assert rc == WW_EUNSUPPORTED and "n_samples" in msg


def test_good_lengths_and_hops_pass_on_to_the_model_check():
    # length and hop valid: the refusal comes from the next check (n_conv 5), before any HIP call, on any machine
    for n, hop in ((4000, 160), (8000, 400), (12000, 160), (15920, 80), (16000, 160), (16380, 4)):
        rc, msg, h = _create_n(2, hop, n, n_conv=5)
        assert rc == WW_EINVAL and "n_conv" in msg and h is None, (n, hop, rc, msg)


def test_detector_takes_half_second_models_and_refuses_longer_than_one_second():
    m = pkg.SimpleWakewordModel(audio_config=_cfg(0.5)).eval()
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.StreamingDetector(m, n_mics=2)
    for d in (0.25, 0.75, 1.0):
        with pytest.raises(RuntimeError, match="no CPU path"):
            pkg.StreamingDetector(pkg.WakewordModel(audio_config=_cfg(d)).eval(), n_mics=2)
    long = pkg.SimpleWakewordModel(audio_config=_cfg(1.5)).eval()
    with pytest.raises(NotImplementedError, match=r"0\.25 \.\. 1 s"):
        pkg.StreamingDetector(long, n_mics=2)


def test_deployment_package_records_the_models_audio_config(tmp_path):
    m = pkg.SimpleWakewordModel(audio_config=_cfg(0.5))
    out = save_deployment_package(m, str(tmp_path / "half.pth"), device="cpu")
    assert out["audio_config"]["DURATION"] == 0.5
    back = torch.load(str(tmp_path / "half.pth"), weights_only=True)
    assert back["audio_config"]["DURATION"] == 0.5
    rebuilt = pkg.SimpleWakewordModel(audio_config=type("Cfg", (AudioConfig,), dict(back["audio_config"])))
    assert rebuilt._n_samples == 8000

    keys = ("SAMPLE_RATE", "DURATION", "N_MELS", "N_FFT", "HOP_LENGTH", "FMIN", "FMAX")
    today = {k: getattr(AudioConfig, k) for k in keys}
    for one in (pkg.SimpleWakewordModel(), pkg.WakewordModel()):
        rec = save_deployment_package(one, str(tmp_path / "one.pth"), device="cpu")["audio_config"]
        assert rec == today and list(rec) == list(keys)
        assert all(type(rec[k]) is type(today[k]) for k in keys)
    full = save_deployment_package(pkg.WakewordModel(audio_config=_cfg(0.75)), str(tmp_path / "full.pth"), device="cpu")
    assert full["audio_config"]["DURATION"] == 0.75
