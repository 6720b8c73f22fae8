"""CPU-only checks of the long-recording scan: the new C entry points are exported and bound and refuse bad
arguments before any HIP call, the Python API refuses bad arguments with ValueError before touching a device, R comes from seconds as
ceil(seconds * 16000 / H), and the numpy restatement of the event rule behaves as the definitions say."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import events_ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import scan

NEW = ("ww_forward_windows_workspace_bytes", "ww_forward_windows_f32", "ww_events_workspace_bytes", "ww_events_sweep_f32",
       "ww_events_state_bytes", "ww_events_step_f32")


def test_abi_stays_4_and_new_symbols_are_bound():
    assert nat.lib.ww_abi_version() == 4 == nat.ABI_VERSION
    lib = C.CDLL(nat.LIB_PATH)
    for name in NEW:
        assert name in nat.PROTOTYPES
        assert hasattr(lib, name)
        assert getattr(nat.lib, name).argtypes == nat.PROTOTYPES[name][1]


def test_lazy_exports():
    assert pkg.scan_files is scan.scan_files and pkg.det_curve is scan.det_curve and pkg.Scan is scan.Scan
    assert pkg.scan is scan


def _err():
    return (nat.lib.ww_last_error() or b"").decode()


def test_c_entry_points_refuse_bad_arguments_before_any_hip_call():
    p = C.c_void_p(16 * 1024)        # never dereferenced: every call below fails its argument check first
    L = nat.lib
    assert L.ww_forward_windows_f32(p, 3, 6, 16000, 1, p, 2, p, 1 << 30, p, None, None) == nat.WW_EINVAL and "hop" in _err()
    assert L.ww_forward_windows_f32(p, 3, 16004, 16000, 1, p, 2, p, 1 << 30, p, None, None) == nat.WW_EINVAL and "hop" in _err()
    assert L.ww_forward_windows_f32(p, 3, 160, 3996, 1, p, 2, p, 1 << 30, p, None, None) == nat.WW_EINVAL and "n_samples" in _err()
    assert L.ww_forward_windows_f32(p, -1, 160, 16000, 1, p, 2, p, 1 << 30, p, None, None) == nat.WW_EINVAL and "n_windows" in _err()
    assert L.ww_forward_windows_f32(p, 3, 160, 16000, 1, p, 4, p, 1 << 30, p, None, None) == nat.WW_EINVAL and "n_conv" in _err()
    assert L.ww_forward_windows_f32(C.c_void_p(16 * 1024 + 4), 3, 160, 16000, 1, p, 2, p, 1 << 30, p, None, None) == nat.WW_EINVAL
    assert "signal_dev" in _err()
    assert L.ww_forward_windows_f32(p, 3, 160, 16000, 1, p, 2, p, 1 << 30, None, None, None) == nat.WW_EINVAL and "logits_dev" in _err()
    assert L.ww_forward_windows_f32(p, 3, 160, 16000, 1, p, 2, p, 100, p, None, None) == nat.WW_EINVAL and "workspace_bytes" in _err()
    assert L.ww_forward_windows_f32(p, 0, 160, 16000, 1, None, 2, None, 0, None, None, None) == nat.WW_OK       # zero windows
    assert L.ww_forward_windows_workspace_bytes(3, 16000, 2) > 0
    assert L.ww_forward_windows_workspace_bytes(3, 16000, 5) == nat.WW_EINVAL

    ws = 1 << 30
    assert L.ww_events_sweep_f32(p, p, 1, 4, 0, 0, p, 1, p, None, p, ws, None) == nat.WW_EINVAL and "smooth" in _err()
    assert L.ww_events_sweep_f32(p, p, 1, 4, 257, 0, p, 1, p, None, p, ws, None) == nat.WW_EINVAL and "smooth" in _err()
    assert L.ww_events_sweep_f32(p, p, 1, 4, 1, -1, p, 1, p, None, p, ws, None) == nat.WW_EINVAL and "refractory" in _err()
    assert L.ww_events_sweep_f32(p, p, 1, 4, 1, 0, p, 0, p, None, p, ws, None) == nat.WW_EINVAL and "n_thr" in _err()
    assert L.ww_events_sweep_f32(p, p, 1, 4, 1, 0, p, 2, p, p, p, ws, None) == nat.WW_EINVAL and "fired_dev" in _err()
    assert L.ww_events_sweep_f32(p, p, -1, 4, 1, 0, p, 1, p, None, p, ws, None) == nat.WW_EINVAL and "n_segs" in _err()
    assert L.ww_events_sweep_f32(p, p, 1, 4, 1, 0, p, 1, None, None, p, ws, None) == nat.WW_EINVAL and "counts_dev" in _err()
    assert L.ww_events_sweep_f32(p, p, 1, 4, 1, 0, p, 1, p, None, p, 8, None) == nat.WW_EINVAL and "workspace_bytes" in _err()
    assert L.ww_events_sweep_f32(None, None, 0, 0, 1, 0, p, 1, None, None, None, 0, None) == nat.WW_OK         # zero segments
    assert L.ww_events_workspace_bytes(10) >= 80

    assert L.ww_events_state_bytes(4, 10) >= 4 * 16 + 4 * 10 * 4
    assert L.ww_events_state_bytes(0, 10) == nat.WW_EINVAL and "n_mics" in _err()
    assert L.ww_events_step_f32(p, 4, 0, 0.5, 0, p, p, None) == nat.WW_EINVAL and "smooth" in _err()
    assert L.ww_events_step_f32(p, 4, 1, 0.0, 0, p, p, None) == nat.WW_EINVAL and "threshold" in _err()
    assert L.ww_events_step_f32(p, 4, 1, 0.5, -3, p, p, None) == nat.WW_EINVAL and "refractory" in _err()
    assert L.ww_events_step_f32(p, 4, 1, 0.5, 0, C.c_void_p(16 * 1024 + 8), p, None) == nat.WW_EINVAL and "state_dev" in _err()
    assert L.ww_events_step_f32(p, 4, 1, 0.5, 0, p, None, None) == nat.WW_EINVAL and "fired_dev" in _err()


def test_refractory_from_seconds():
    assert scan.refractory_windows(1.0, 160) == 100
    assert scan.refractory_windows(0.0, 160) == 0
    assert scan.refractory_windows(0.001, 160) == 1              # 0.1 window -> 1
    assert scan.refractory_windows(1.0, 512) == math.ceil(16000 / 512) == 32
    assert scan.refractory_windows(0.5, 400) == 20
    for bad in (-0.1, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError):
            scan.refractory_windows(bad, 160)


def _model(train=False, n=16000):
    cfg = type("Cfg", (pkg.AudioConfig,), {"DURATION": n / 16000.0})
    m = pkg.SimpleWakewordModel(audio_config=cfg)
    return m.train() if train else m.eval()


def test_scan_files_refuses_bad_arguments_before_the_device():
    with pytest.raises(NotImplementedError):
        scan.scan_files(_model(train=True), [])
    m = _model()
    for hop in (0, 2, 6, 16004, 160.0, True):
        with pytest.raises(ValueError):
            scan.scan_files(m, [], hop_samples=hop)
    with pytest.raises(ValueError):
        scan.scan_files(_model(n=8000), [], hop_samples=8004)     # H <= N of the model
    for bs in (0, -1, 1.5):
        with pytest.raises(ValueError):
            scan.scan_files(m, [], batch_size=bs)
    with pytest.raises(ValueError):
        scan.scan_files(m, "one_file.wav")
    with pytest.raises(RuntimeError):                              # CPU parameters: no CPU path, and no device was touched before
        scan.scan_files(m, [], hop_samples=160)


def _cpu_scan(prob, lengths, hop=160, window=16000):
    return scan.Scan(torch.as_tensor(np.asarray(prob, np.float32)), lengths, [f"f{i}" for i in range(len(lengths))], [], hop, window, None,
                     torch.device("cpu"))


def test_scan_methods_refuse_bad_arguments():
    s = _cpu_scan(np.zeros(7), [1000, 120])
    assert s.window_offsets.tolist() == [0, 7, 8] and s.offsets.tolist() == [0, 1000]
    assert s.hours == pytest.approx(1120 / 16000 / 3600)
    for kw in ({"smooth": 0}, {"smooth": 257}, {"smooth": 2.5}, {"refractory_s": -1}, {"refractory_s": float("nan")}):
        with pytest.raises(ValueError):
            s.counts([0.5], **kw)
        with pytest.raises(ValueError):
            s.events(0.5, **kw)
    for thr in ([], [0.0], [1.5], [-0.1], [float("nan")], np.full(65537, 0.5)):
        with pytest.raises(ValueError):
            s.counts(thr)
    for thr in (0.0, 1.01):
        with pytest.raises(ValueError):
            s.events(thr)
    with pytest.raises(ValueError):
        s.hard_negatives(0.5)                                       # no audio kept


def test_det_curve_refuses_bad_arguments_before_the_device():
    m = _model()
    with pytest.raises(ValueError):
        scan.det_curve(m, [], [], thresholds=[0.0, 0.5])
    with pytest.raises(ValueError):
        scan.det_curve(m, [], [], smooth=0)
    with pytest.raises(ValueError):
        scan.det_curve(m, [], [], hop_samples=162)
    with pytest.raises(ValueError):
        scan.det_curve(m, [], [], refractory_s=-1)


def test_streaming_detector_event_arguments_are_checked_first():
    m = _model()
    for kw in ({"smooth": 0}, {"smooth": 300}, {"smooth": 1.5}, {"refractory_s": -1.0}, {"refractory_s": float("inf")},
               {"smooth": 2, "threshold": 0.0}, {"refractory_s": 1.0, "threshold": 1.5}):
        with pytest.raises(ValueError):
            pkg.StreamingDetector(m, n_mics=2, hop_samples=160, **kw)
    with pytest.raises(RuntimeError):                              # valid arguments: then the CPU model is refused, as before
        pkg.StreamingDetector(m, n_mics=2, hop_samples=160, smooth=3, refractory_s=0.5)
    with pytest.raises(NotImplementedError):
        pkg.StreamingDetector(_model(train=True), smooth=3)


def test_det_curve_threshold_for_picks_the_lowest_qualifying_threshold():
    c = scan.DetCurve(thresholds=np.array([0.1, 0.2, 0.3, 0.4], np.float32), fa_per_hour=np.array([3.0, 0.5, 0.2, 0.0]),
                      frr=np.zeros(4), negative_hours=1.0, n_positive=0, unreadable=[])
    assert c.threshold_for(0.5) == pytest.approx(0.2)
    assert c.threshold_for(0.25) == pytest.approx(0.3)
    assert c.threshold_for(10) == pytest.approx(0.1)
    assert c.threshold_for(-1) is None
    assert scan.threshold_for(dict(c), 0.0) == pytest.approx(0.4)


def test_restatement_follows_the_definitions():
    p = np.array([0.2, np.nan, 0.9, 0.9, 0.1, 0.95, 0.95, 0.95], np.float32)
    s1 = events_ref.smooth(p, 1)
    assert np.array_equal(s1, np.where(np.isfinite(p), p, 0).astype(np.float64))
    s3 = events_ref.smooth(p, 3)
    q = np.where(np.isfinite(p), p, 0).astype(np.float64)
    assert s3[0] == q[0] and s3[1] == (q[0] + q[1]) / 2 and s3[4] == ((q[2] + q[3]) + q[4]) / 3
    f = events_ref.fired(s1, [0.9], 1)[0]
    assert f.tolist() == [False, False, True, False, False, True, False, True]       # k - k_last > R: 2 -> 5 -> 7 (7 - 5 = 2 > 1)
    f = events_ref.fired(s1, [0.9], 2)[0]
    assert f.tolist() == [False, False, True, False, False, True, False, False]      # 7 - 5 = 2 is not > 2
    assert events_ref.counts(p, [0, 0, 3, 8], [0.9, 0.95], 1, 0).tolist() == [[0, 0], [1, 0], [4, 3]]
    w = events_ref.windows(np.arange(1, 11, dtype=np.float32), 8, 4)
    assert w.shape == (3, 8)
    assert w[0].tolist() == [0, 0, 0, 0, 1, 2, 3, 4] and w[2].tolist() == [5, 6, 7, 8, 9, 10, 0, 0]
    assert events_ref.windows(np.zeros(0, np.float32), 8, 4).shape == (0, 8)
