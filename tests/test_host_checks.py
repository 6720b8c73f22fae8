"""The tensor checks of ops.py without a GPU: one check each for pcm rows, mel images and pooled features, shared by the public
functions and the raw launches (`_*_impl`), so both refuse a bad tensor with the same exception type and the same message, before any
device call.  A CPU tensor is refused for its device first; to reach the checks behind that one, `OnGpu` reports a GPU as its device
while its memory stays on the host -- every case here is refused, so nothing ever dereferences it."""
import pytest
import torch

from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import ops


class OnGpu(torch.Tensor):
    device = property(lambda self: torch.device("cuda", 0))


def on_gpu(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(OnGpu)


def packed(n_conv):
    return on_gpu(nat.lib.ww_packed_weights_floats(n_conv))


def refusal(fn, *args):
    with pytest.raises(Exception) as e:
        fn(*args)
    return type(e.value), str(e.value)


# what is wrong -> (exception, a word of the message, the tensor)
BAD_PCM = {
    "device": (RuntimeError, "no CPU implementation", lambda: torch.zeros(2, 16000)),
    "dtype": (TypeError, "expected float32", lambda: on_gpu(2, 16000, dtype=torch.float64)),
    "rank": (ValueError, "expected [B, samples]", lambda: on_gpu(2, 1, 16000)),
    "no samples": (ValueError, "0 samples per clip", lambda: on_gpu(2, 0)),
    "too many samples": (ValueError, "16001 samples per clip; the front-end takes 1..16000", lambda: on_gpu(2, 16001)),
}
BAD_X = {
    "device": (RuntimeError, "no CPU implementation", lambda: torch.zeros(2, 1, 80, 32)),
    "dtype": (TypeError, "expected float32", lambda: on_gpu(2, 1, 80, 32, dtype=torch.float16)),
    "rank": (ValueError, "expected [B, 1, 80, T]", lambda: on_gpu(2, 80, 32)),
    "mel bins": (ValueError, "expected [B, 1, 80, T]", lambda: on_gpu(2, 1, 64, 32)),
    "no frames": (NotImplementedError, "T = 0 frames", lambda: on_gpu(2, 1, 80, 0)),
    "too many frames": (NotImplementedError, "T = 33 frames; the conv kernels are built for 1..32", lambda: on_gpu(2, 1, 80, 33)),
}
BAD_POOLED = {
    "device": (RuntimeError, "no CPU implementation", lambda: torch.zeros(2, 64)),
    "dtype": (TypeError, "expected float32", lambda: on_gpu(2, 64, dtype=torch.int32)),
    "rank": (ValueError, "pooled: expected [B, 64]", lambda: on_gpu(2, 64, 1)),
    "channels": (ValueError, "pooled: expected [B, 64]", lambda: on_gpu(2, 128)),
}


@pytest.mark.parametrize("what", sorted(BAD_PCM))
def test_pcm_is_refused_alike_by_public_and_impl(what):
    exc, word, make = BAD_PCM[what]
    pcm, w = make(), packed(2)
    got = refusal(ops.logmel, pcm)
    assert got[0] is exc and word in got[1], got
    assert refusal(ops._logmel_impl, pcm) == got
    assert refusal(ops.forward_pcm, pcm, w, 2) == got and refusal(ops._forward_pcm_impl, pcm, w, 2) == got


@pytest.mark.parametrize("what", sorted(BAD_X))
def test_mel_images_are_refused_alike_by_public_and_impl(what):
    exc, word, make = BAD_X[what]
    x, w = make(), packed(2)
    got = refusal(ops.cnn_pool, x, w, 2)
    assert got[0] is exc and word in got[1], got
    assert refusal(ops._cnn_pool_impl, x, w, 2) == got
    assert refusal(ops.cnn_lstm_forward, x, w, 2) == got and refusal(ops._cnn_lstm_forward_impl, x, w, 2) == got
    assert refusal(ops._check_x, x) == got


@pytest.mark.parametrize("what", sorted(BAD_POOLED))
def test_pooled_is_refused_alike_by_public_and_impl(what):
    exc, word, make = BAD_POOLED[what]
    pooled, w = make(), packed(2)
    got = refusal(ops.lstm_fc, pooled, w, 2)
    assert got[0] is exc and word in got[1], got
    assert refusal(ops._lstm_fc_impl, pooled, w, 2) == got


def test_the_frame_limit_is_the_callers():
    """The same check with another limit: the column-tiled conv stack takes 63 frames and says so; the *_frames functions bound the
    samples by their clip length."""
    w = packed(3)
    assert refusal(ops.cnn_pool_wide, on_gpu(2, 1, 80, 64), w, 3) == (
        NotImplementedError, "x: T = 64 frames; the conv kernels take 1..63 (2 s clips give 63)")
    assert refusal(ops.cnn_pool_wide, on_gpu(2, 80, 63), w, 3) == refusal(ops.cnn_pool, on_gpu(2, 80, 63), w, 3)
    for fn, args in ((ops.logmel_frames, (8000,)), (ops.forward_pcm_frames, (w, 3, 8000))):
        assert refusal(fn, on_gpu(2, 8001), *args) == (
            ValueError, "pcm: 8001 samples per clip; this clip length takes 1..8000 (crop longer clips on the host)")
        assert refusal(fn, on_gpu(2, 0), *args)[0] is ValueError
        assert refusal(fn, on_gpu(2, 8000, dtype=torch.float64), *args) == refusal(ops.logmel, on_gpu(2, 8000, dtype=torch.float64))
    assert refusal(ops.logmel_frames, on_gpu(2, 100), 3999)[0] is NotImplementedError


@pytest.mark.parametrize("fn,hi,args", [(ops.augment, 16383, ([],)), (ops.augment_stages, 16383, ([],)), (ops.mix_background, 32000, (None, 0, 0, 0.0)),
                                        (ops.reverb, 32000, (None, 0))])
def test_augmentation_clips_are_refused_with_the_functions_name_and_range(fn, hi, args):
    name = fn.__name__
    rows = "B >= 1" if fn is ops.augment_stages else "B"
    assert refusal(fn, torch.zeros(2, 8000), *args) == (RuntimeError, f"{name}: pcm must live on the MI355X (no CPU fallback)")
    for bad in (on_gpu(2, 8000, dtype=torch.float64), on_gpu(8000), on_gpu(2, 3999), on_gpu(2, hi + 1)):
        assert refusal(fn, bad, *args) == (
            ValueError, f"{name}: expected float32 [{rows}, N], N in 4000..{hi}, got {bad.dtype} {tuple(bad.shape)}")
    if fn is ops.augment_stages:
        assert refusal(fn, on_gpu(0, 8000), *args)[1] == "augment_stages: expected float32 [B >= 1, N], N in 4000..16383, got torch.float32 (0, 8000)"
