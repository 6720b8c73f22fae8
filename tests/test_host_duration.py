"""Clip lengths from 0.25 s to 2 s, host side (no GPU): the config bounds, the argument checks of the new C entry points, the Meta
kernels' shapes, the reader's clip length, and the refusals of what stays 1 s only (training, augmentation, streaming)."""
import numpy as np
import pytest
import torch

import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import ops
from wakeword_jupyterlab_amd.config import AudioConfig, check_audio_config, n_frames, n_samples


def _cfg(duration, **kw):
    return type("Cfg", (AudioConfig,), {"DURATION": duration, **kw})


def test_config_bounds_and_frame_counts():
    for d, n, t in ((0.25, 4000, 8), (0.5, 8000, 16), (1.0, 16000, 32), (1.5, 24000, 47), (2.0, 32000, 63)):
        check_audio_config(_cfg(d))
        assert n_samples(_cfg(d)) == n and n_frames(_cfg(d)) == t
        assert pkg.WakewordModel(audio_config=_cfg(d)).mel_width == t       # the reference's own formula agrees
    for d in (0.2, 2.1, 3.0):
        with pytest.raises(NotImplementedError):
            check_audio_config(_cfg(d))
        with pytest.raises(NotImplementedError):
            pkg.AudioProcessor(_cfg(d))
    with pytest.raises(NotImplementedError):
        check_audio_config(_cfg(1.5, N_FFT=1024))
    with pytest.raises(NotImplementedError):
        check_audio_config(_cfg(1.0, HOP_LENGTH=256))


def test_new_entry_points_refuse_bad_arguments_before_touching_a_device():
    L = nat.lib
    p = C_void = None
    # n_samples beyond 2 s / below 0.25 s, clip_len > n_samples
    assert L.ww_logmel_frames_f32(p, 1, 32004, 32001, 32001, 1, C_void, None) == nat.WW_EINVAL
    assert L.ww_logmel_frames_f32(p, 1, 3996, 3999, 3999, 1, C_void, None) == nat.WW_EINVAL
    assert L.ww_logmel_frames_f32(p, 1, 24000, 24001, 24000, 1, C_void, None) == nat.WW_EINVAL
    assert L.ww_forward_pcm_frames_f32(p, 1, 32004, 32001, 32001, 1, p, 2, p, p, None) == nat.WW_EINVAL
    assert L.ww_forward_pcm_frames_f32(p, 1, 24000, 24001, 24000, 1, p, 2, p, p, None) == nat.WW_EINVAL
    assert L.ww_workspace_frames_bytes(8, 32001, 2) == nat.WW_EINVAL
    assert L.ww_decode_resample_n(p, p, 1, 1, 32001, p, None) == nat.WW_EINVAL
    assert L.ww_decode_resample_n(p, p, 1, 1, 3999, p, None) == nat.WW_EINVAL
    assert L.ww_wav_batch_decode_n(p, 0, 1, 40000, p, None) == nat.WW_EINVAL
    # 64 frames
    assert L.ww_cnn_pool_wide_f32(p, 1, 64, p, 2, p, p, None) == nat.WW_EINVAL
    assert L.ww_cnn_pool_wide_f32(p, 1, 0, p, 3, p, p, None) == nat.WW_EINVAL
    assert L.ww_cnn_wide_scratch_bytes(8, 64, 2) == nat.WW_EINVAL
    assert L.ww_cnn_wide_scratch_bytes(8, 63, 4) == nat.WW_EINVAL
    # the 1 s entry points keep their limits
    assert L.ww_logmel_f32(p, 1, 20000, 20000, 1, p, None) == nat.WW_EINVAL
    assert L.ww_cnn_pool_f32(p, 1, 33, p, 2, p, p, None) == nat.WW_EUNSUPPORTED


def test_scratch_sizes_follow_the_tiling():
    L = nat.lib
    assert L.ww_cnn_wide_scratch_bytes(10, 32, 3) == L.ww_cnn_scratch_bytes(10, 3)      # <= 32 columns: the 1 s kernels
    assert L.ww_cnn_wide_scratch_bytes(10, 20, 2) == 0
    # 2-conv: 2 tiles at T = 47, 3 at T = 63 -> partial pools only; 3-conv: also relu(conv2) per tile
    assert L.ww_cnn_wide_scratch_bytes(10, 47, 2) == 20 * 64 * 4
    assert L.ww_cnn_wide_scratch_bytes(10, 63, 2) == 30 * 64 * 4
    assert L.ww_cnn_wide_scratch_bytes(10, 63, 3) >= 30 * 80 * 64 * 32 * 4
    assert L.ww_workspace_frames_bytes(4, 24000, 3) > L.ww_workspace_frames_bytes(4, 24000, 2) > 0


def test_meta_kernels_give_the_shapes():
    for n in (4000, 16000, 24000, 32000):
        T = 1 + n // 512
        pcm = torch.empty(5, n - 3, device="meta")
        assert torch.ops.wakeword_amd.logmel_frames(pcm, n, True).shape == (5, 1, 80, T)
        assert torch.ops.wakeword_amd.forward_pcm_frames(pcm, torch.empty(10, device="meta"), 3, n, True).shape == (5, 2)
    for T, nc, c in ((33, 2, 64), (63, 3, 128), (8, 2, 64)):
        x = torch.empty(7, 1, 80, T, device="meta")
        assert torch.ops.wakeword_amd.cnn_pool_wide(x, torch.empty(10, device="meta"), nc).shape == (7, c)
    with pytest.raises(RuntimeError):
        torch.ops.wakeword_amd.cnn_pool_wide(torch.empty(1, 1, 80, 64, device="meta"), torch.empty(1, device="meta"), 2)
    with pytest.raises(RuntimeError):
        torch.ops.wakeword_amd.logmel_frames(torch.empty(1, 100, device="meta"), 32256, True)


def test_the_new_ops_have_no_cpu_path():
    with pytest.raises(RuntimeError):
        torch.ops.wakeword_amd.logmel_frames(torch.zeros(1, 100), 24000, True)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        ops.cnn_pool_wide(torch.zeros(1, 1, 80, 47), torch.zeros(10), 2)


def test_training_augmentation_and_streaming_stay_one_second():
    cfg = _cfg(1.5)
    m = pkg.WakewordModel(audio_config=cfg)
    m.train()
    with pytest.raises(NotImplementedError, match="training"):
        m(torch.zeros(2, 1, 80, 47))
    s = pkg.SimpleWakewordModel(audio_config=cfg)
    s.train()
    with pytest.raises(NotImplementedError, match="training"):
        s(torch.zeros(2, 1, 80, 33))
    s.eval()
    with pytest.raises(NotImplementedError):
        pkg.StreamingDetector(s, n_mics=2)
    proc = pkg.AudioProcessor(cfg)
    with pytest.raises(NotImplementedError, match="augmentation"):
        proc.augment_audio(np.zeros(24000, np.float32))
    with pytest.raises(NotImplementedError, match="augmentation"):
        proc.process_audio_file("missing.wav", augment=True)
    assert pkg.SimpleWakewordModel()._max_width == 32 and pkg.SimpleWakewordModel(audio_config=_cfg(2.0))._max_width == 63


def test_reader_crops_against_the_configured_clip_length():
    import random
    from wakeword_jupyterlab_amd.files import DESC_DTYPE, WavBatchReader
    with pytest.raises(NotImplementedError):
        WavBatchReader(host_only=True, n_samples=40000)
    r = WavBatchReader(max_clips=4, host_only=True, n_samples=24000)
    try:
        assert r.n_samples == 24000
        r.regrow(8, r.max_raw_bytes)
        assert r.n_samples == 24000 and r.max_clips == 8        # a regrown reader keeps its clip length
    finally:
        r.close()
    d = np.zeros(3, dtype=DESC_DTYPE)
    d["n_frames"] = [30000, 24000, 48000]
    d["up"] = d["down"] = 1
    random.seed(4)
    WavBatchReader.draw_crops(d, np.ones(3, np.int8), 24000)
    rr = random.Random(4)
    assert list(d["crop_start"]) == [rr.randint(0, 6000), 0, rr.randint(0, 24000)]
