"""Tensor-level entry points: torch custom ops (`torch.ops.wakeword_amd.*`) over the C ABI.

PyTorch is plumbing here (device memory, the current HIP stream, op registration); the arithmetic is
in libwakeword_amd.so.  Every op checks shape / dtype / device, launches on torch's current stream,
never synchronises and never falls back to a CPU implementation.

  logmel(pcm[B,n<=16000] f32, normalize)            -> [B,1,80,32]   (SURVEY.md boundary B1)
  cnn_lstm_forward(x[B,1,80,T<=32], packed, n_conv) -> [B,2]         (boundary B2)
  forward_pcm(pcm[B,n], packed, n_conv, normalize)  -> [B,2]         (boundary B3)
  cnn_pool / lstm_fc                                 the two halves of B2, exposed for tests and profiling
"""
from __future__ import annotations

import ctypes as C
import os
import weakref

import numpy as np
import torch

from . import _native as nat
from .config import (CHANNEL_MAX_DRIVE, CHANNEL_MAX_HZ, CHANNEL_MAX_PEAKS, CHANNEL_SECTIONS, CLIP_SAMPLES, N_FRAMES, SPEC_MAX_MASKS, AudioConfig,
                     ChannelConfig, SpecAugmentConfig, check_channel_config, check_spec_augment_config)

N_MELS = AudioConfig.N_MELS
MAX_FRAMES = 63                         # 1 + 32000 // 512
MIN_CLIP_SAMPLES, MAX_CLIP_SAMPLES = 4000, 32000


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


def _require_cuda_f32(t: torch.Tensor, name: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name} is on {t.device}: this path has no CPU implementation; move it to the MI355X (`.cuda()`)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")


def c_last(n_conv: int) -> int:
    return {2: 64, 3: 128}[n_conv]


# ------------------------------------------------------------------------------------------------
# weights
# ------------------------------------------------------------------------------------------------
def pack_state_dict(state_dict) -> np.ndarray:
    """Reference state_dict (torch tensors or numpy arrays, torch layout) -> packed float32 image (host).

    Accepts the key set of SimpleWakewordModel (train_wakeword.py:28-36) or WakewordModel
    (wakeword_training_script.py:141-165); `lstm.weight_hh_l*` may be present and is ignored (it is
    mathematically dead on this path)."""
    def arr(key, shape):
        if key not in state_dict:
            raise KeyError(f"state_dict is missing '{key}'")
        v = state_dict[key]
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        v = np.ascontiguousarray(v, dtype=np.float32)
        if tuple(v.shape) != tuple(shape):
            raise ValueError(f"{key}: shape {tuple(v.shape)} != expected {tuple(shape)}")
        return v

    n_conv = 3 if "conv3.weight" in state_dict else 2
    chans = [1, 32, 64, 128][: n_conv + 1]
    keep = []
    sd = nat.StateDict()
    sd.n_conv, sd.hidden = n_conv, 256
    for i in range(n_conv):
        w = arr(f"conv{i + 1}.weight", (chans[i + 1], chans[i], 3, 3)); b = arr(f"conv{i + 1}.bias", (chans[i + 1],))
        keep += [w, b]
        sd.conv_weight[i], sd.conv_bias[i] = w.ctypes.data, b.ctypes.data
    for layer, nin in enumerate([chans[-1], 256]):
        w = arr(f"lstm.weight_ih_l{layer}", (1024, nin))
        bi = arr(f"lstm.bias_ih_l{layer}", (1024,)); bh = arr(f"lstm.bias_hh_l{layer}", (1024,))
        keep += [w, bi, bh]
        sd.lstm_weight_ih[layer], sd.lstm_bias_ih[layer], sd.lstm_bias_hh[layer] = w.ctypes.data, bi.ctypes.data, bh.ctypes.data
    fw = arr("fc.weight", (2, 256)); fb = arr("fc.bias", (2,))
    keep += [fw, fb]
    sd.fc_weight, sd.fc_bias = fw.ctypes.data, fb.ctypes.data
    out = np.empty(nat.check(nat.lib.ww_packed_weights_floats(n_conv)), dtype=np.float32)
    nat.check(nat.lib.ww_pack_weights_host(C.byref(sd), out.ctypes.data))
    return out


def n_conv_of_packed(packed: torch.Tensor) -> int:
    for n_conv in (2, 3):
        if packed.numel() == nat.lib.ww_packed_weights_floats(n_conv):
            return n_conv
    raise ValueError(f"packed weight image of {packed.numel()} floats matches neither model")


# ------------------------------------------------------------------------------------------------
# raw launches (plain functions; the registered custom ops below wrap them)
# ------------------------------------------------------------------------------------------------
def frames_of(n_samples: int) -> int:
    if not MIN_CLIP_SAMPLES <= int(n_samples) <= MAX_CLIP_SAMPLES:
        raise NotImplementedError(f"clips of {n_samples} samples: the front-end takes {MIN_CLIP_SAMPLES}..{MAX_CLIP_SAMPLES} (0.25 s .. 2 s)")
    return 1 + int(n_samples) // 512


# The tensor checks, one each for pcm rows, mel images and pooled features: TypeError / ValueError / NotImplementedError before any device
# call.  The public functions and the raw launches (`_*_impl`) share them; the compiled operators re-check with TORCH_CHECK -> RuntimeError.
def _require_pcm(pcm, n_samples=None) -> None:
    """pcm [B, 1..limit] float32 on the GPU; the limit is one second, or `n_samples` (0.25 s .. 2 s) for the *_frames functions."""
    if n_samples is not None:
        frames_of(n_samples)
    _require_cuda_f32(pcm, "pcm")
    if pcm.dim() != 2:
        raise ValueError(f"pcm: expected [B, samples], got {tuple(pcm.shape)}")
    if pcm.shape[1] == 0 or pcm.shape[1] > (CLIP_SAMPLES if n_samples is None else n_samples):
        raise ValueError(f"pcm: {pcm.shape[1]} samples per clip; " +
                         (f"the front-end takes 1..{CLIP_SAMPLES} (crop longer clips on the host, pad_or_truncate "
                          "wakeword_training_script.py:78-83)" if n_samples is None else
                          f"this clip length takes 1..{n_samples} (crop longer clips on the host)"))


def _require_x(x, max_frames: int = 32) -> None:
    """x [B, 1, 80, 1..max_frames] float32 on the GPU: 32 frames for the conv kernels, MAX_FRAMES for their column-tiled form."""
    _require_cuda_f32(x, "x")
    if x.dim() != 4 or x.shape[1] != 1 or x.shape[2] != N_MELS:
        raise ValueError(f"x: expected [B, 1, {N_MELS}, T], got {tuple(x.shape)}")
    if not 1 <= x.shape[3] <= max_frames:
        raise NotImplementedError(f"x: T = {x.shape[3]} frames; the conv kernels " +
                                  ("are built for 1..32 (1 s clips give 32)" if max_frames == 32 else f"take 1..{max_frames} (2 s clips give 63)"))


def _require_pooled(pooled, packed, n_conv) -> None:
    _require_cuda_f32(pooled, "pooled")
    _check_packed(packed, n_conv, pooled)
    if pooled.dim() != 2 or pooled.shape[1] != c_last(n_conv):
        raise ValueError(f"pooled: expected [B, {c_last(n_conv)}], got {tuple(pooled.shape)}")


def _check_pcm(pcm: torch.Tensor) -> torch.Tensor:
    _require_pcm(pcm)
    return _aligned_rows(pcm)


def _aligned_rows(pcm: torch.Tensor) -> torch.Tensor:
    """The rows as the native entry points take them: 16-byte aligned, row stride a multiple of 4 floats (copied only when needed)."""
    if pcm.stride(1) != 1 or (pcm.shape[0] > 1 and pcm.stride(0) % 4) or pcm.data_ptr() % 16:
        pcm = pcm.contiguous()
        if pcm.shape[1] % 4 and pcm.shape[0] > 1:      # row stride must be a multiple of 4 floats
            pad = torch.zeros(pcm.shape[0], (pcm.shape[1] + 3) // 4 * 4, device=pcm.device, dtype=pcm.dtype)
            pad[:, : pcm.shape[1]] = pcm
            pcm = pad[:, : pcm.shape[1]]
    return pcm


def _logmel_impl(pcm: torch.Tensor, normalize: bool = True) -> torch.Tensor:
    pcm = _check_pcm(pcm)
    B, n = pcm.shape
    out = torch.empty((B, 1, N_MELS, N_FRAMES), device=pcm.device, dtype=torch.float32)
    with torch.cuda.device(pcm.device):
        nat.check(nat.lib.ww_logmel_f32(_ptr(pcm), B, pcm.stride(0) if B > 1 else n, n, int(bool(normalize)), _ptr(out), _stream()))
    return out


def _check_x(x: torch.Tensor) -> torch.Tensor:
    _require_x(x)
    return x.contiguous()


def _check_packed(packed: torch.Tensor, n_conv: int, like: torch.Tensor) -> None:
    _require_cuda_f32(packed, "packed weights")
    if packed.device != like.device:
        raise RuntimeError(f"packed weights on {packed.device}, input on {like.device}")
    if n_conv not in (2, 3) or packed.numel() != nat.lib.ww_packed_weights_floats(n_conv) or not packed.is_contiguous():
        raise ValueError("packed weights do not match n_conv (use ops.pack_state_dict)")


def _cnn_pool_impl(x: torch.Tensor, packed: torch.Tensor, n_conv: int) -> torch.Tensor:
    x = _check_x(x)
    _check_packed(packed, n_conv, x)
    B, T = x.shape[0], x.shape[3]
    pooled = torch.empty((B, c_last(n_conv)), device=x.device, dtype=torch.float32)
    nbytes = nat.check(nat.lib.ww_cnn_scratch_bytes(B, n_conv))
    scratch = torch.empty(nbytes, device=x.device, dtype=torch.uint8) if nbytes else None
    with torch.cuda.device(x.device):
        nat.check(nat.lib.ww_cnn_pool_f32(_ptr(x), B, T, _ptr(packed), n_conv, _ptr(scratch) if nbytes else None, _ptr(pooled), _stream()))
    return pooled


def _lstm_fc_impl(pooled: torch.Tensor, packed: torch.Tensor, n_conv: int) -> torch.Tensor:
    _require_pooled(pooled, packed, n_conv)
    pooled = pooled.contiguous()
    logits = torch.empty((pooled.shape[0], 2), device=pooled.device, dtype=torch.float32)
    with torch.cuda.device(pooled.device):
        nat.check(nat.lib.ww_lstm_fc_f32(_ptr(pooled), pooled.shape[0], _ptr(packed), n_conv, _ptr(logits), _stream()))
    return logits


def _workspace(n: int, n_conv: int, device) -> torch.Tensor:
    return torch.empty(max(1, nat.check(nat.lib.ww_workspace_bytes(n, n_conv))), device=device, dtype=torch.uint8)


def _cnn_lstm_forward_impl(x: torch.Tensor, packed: torch.Tensor, n_conv: int) -> torch.Tensor:
    x = _check_x(x)
    _check_packed(packed, n_conv, x)
    B, T = x.shape[0], x.shape[3]
    logits = torch.empty((B, 2), device=x.device, dtype=torch.float32)
    ws = _workspace(B, n_conv, x.device)
    with torch.cuda.device(x.device):
        nat.check(nat.lib.ww_model_forward_f32(_ptr(x), B, T, _ptr(packed), n_conv, _ptr(ws), _ptr(logits), _stream()))
    return logits


def forward_workspace_bytes(B: int, n_conv: int) -> int:
    """ww_workspace_bytes: what ww_model_forward_f32 needs for B clips (at least 1, so that a buffer of this size has a pointer)."""
    return max(1, nat.check(nat.lib.ww_workspace_bytes(B, n_conv)))


def model_forward_into(x, packed, n_conv: int, ws, logits) -> None:
    """ww_model_forward_f32, the eval-mode chain of cnn_lstm_forward, on caller-owned buffers: x as _check_x returns it (T <= 32), `packed`
    as model.packed_weights() gives it, `ws` uint8 of at least forward_workspace_bytes(B, n_conv), logits float32 [>= B, 2] contiguous.
    One native call on the current stream of the CURRENT device, which the caller has made x's; allocates nothing."""
    nat.check(nat.lib.ww_model_forward_f32(_ptr(x), x.shape[0], x.shape[3], _ptr(packed), n_conv, _ptr(ws), _ptr(logits), _stream()))


def _forward_pcm_impl(pcm: torch.Tensor, packed: torch.Tensor, n_conv: int, normalize: bool = True) -> torch.Tensor:
    pcm = _check_pcm(pcm)
    _check_packed(packed, n_conv, pcm)
    B, n = pcm.shape
    logits = torch.empty((B, 2), device=pcm.device, dtype=torch.float32)
    ws = _workspace(B, n_conv, pcm.device)
    with torch.cuda.device(pcm.device):
        nat.check(nat.lib.ww_forward_pcm_f32(_ptr(pcm), B, pcm.stride(0) if B > 1 else n, n, int(bool(normalize)),
                                             _ptr(packed), n_conv, _ptr(ws), _ptr(logits), _stream()))
    return logits


# ------------------------------------------------------------------------------------------------
# torch custom ops: torch.ops.wakeword_amd.{logmel,cnn_pool,lstm_fc,cnn_lstm_forward,forward_pcm}
# ------------------------------------------------------------------------------------------------
# COMPILED operators (csrc/ww_torch_ops.cpp -> libwakeword_amd_torch.so: TORCH_LIBRARY schema + CUDA, Meta and CPU kernels, SURVEY.md
# section 7 step 2).  The CUDA kernels validate, allocate with ATen and call the C ABI on torch's current stream; the Meta kernels give
# shapes only (FakeTensor / torch.compile tracing of the drop-in modules); the CPU kernels refuse.  Rounds 1-3 registered the Python
# functions above through torch.library; those stay as plain functions (`_logmel_impl` ...: tests and the raw launches of bench.py's legs).
# The library does not link libwakeword_amd.so: it is handed the addresses of the sixteen C ABI functions it calls.
# No fallback: without the compiled library the package does not import.
TORCH_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libwakeword_amd_torch.so")
if not os.path.exists(TORCH_LIB_PATH):
    raise ImportError(f"{TORCH_LIB_PATH} is missing: build it with `make -C wakeword-jupyterlab_amd/csrc` "
                      "(or `python -c 'import __graft_entry__ as g; g.build()'`)")
torch.ops.load_library(TORCH_LIB_PATH)
# bind the operators to THE copy of libwakeword_amd.so this process uses (the shipped one or a WW_LIB_OVERRIDE build): addresses, not names
_TORCH_BIND_ORDER = ("ww_last_error", "ww_packed_weights_floats", "ww_cnn_scratch_bytes", "ww_workspace_bytes", "ww_logmel_f32",
                     "ww_cnn_pool_f32", "ww_lstm_fc_f32", "ww_model_forward_f32", "ww_forward_pcm_f32",
                     "ww_logmel_frames_f32", "ww_cnn_wide_scratch_bytes", "ww_cnn_pool_wide_f32", "ww_workspace_frames_bytes",
                     "ww_forward_pcm_frames_f32", "ww_spec_augment_f32", "ww_channel_f32")
_torch_lib = C.CDLL(TORCH_LIB_PATH)
_table = (C.c_void_p * len(_TORCH_BIND_ORDER))(*[C.cast(getattr(nat.lib, _n), C.c_void_p).value for _n in _TORCH_BIND_ORDER])
if _torch_lib.ww_torch_bind(_table, len(_TORCH_BIND_ORDER)) != 0:
    raise ImportError("libwakeword_amd_torch.so refused the C ABI table (rebuild: make -C wakeword-jupyterlab_amd/csrc)")


# The public functions run the shared checks above first (the messages rounds 1-3 gave), then dispatch: real tensors reach the HIP kernels,
# fake / meta tensors the shape-only kernels.
def logmel(pcm: torch.Tensor, normalize: bool = True) -> torch.Tensor:
    _require_pcm(pcm)
    return torch.ops.wakeword_amd.logmel(pcm, bool(normalize))


def cnn_pool(x, packed, n_conv):
    _require_x(x)
    _check_packed(packed, n_conv, x)
    return torch.ops.wakeword_amd.cnn_pool(x, packed, n_conv)


def lstm_fc(pooled, packed, n_conv):
    _require_pooled(pooled, packed, n_conv)
    return torch.ops.wakeword_amd.lstm_fc(pooled, packed, n_conv)


def cnn_lstm_forward(x, packed, n_conv):
    _require_x(x)
    _check_packed(packed, n_conv, x)
    return torch.ops.wakeword_amd.cnn_lstm_forward(x, packed, n_conv)


def forward_pcm(pcm, packed, n_conv, normalize: bool = True):
    _require_pcm(pcm)
    _check_packed(packed, n_conv, pcm)
    return torch.ops.wakeword_amd.forward_pcm(pcm, packed, n_conv, bool(normalize))


# ---- clips of 0.25 s .. 2 s (inference): torch.ops.wakeword_amd.{logmel_frames,cnn_pool_wide,forward_pcm_frames} ----
def logmel_frames(pcm: torch.Tensor, n_samples: int, normalize: bool = True) -> torch.Tensor:
    """pcm [B, n <= n_samples] -> [B, 1, 80, T], T = 1 + n_samples // 512: the log-mel of clips zero-padded to n_samples.
    n_samples = 16000 gives exactly `logmel`'s result."""
    _require_pcm(pcm, n_samples)
    return torch.ops.wakeword_amd.logmel_frames(pcm, int(n_samples), bool(normalize))


def cnn_pool_wide(x, packed, n_conv):
    """x [B, 1, 80, T], 1 <= T <= 63 -> pooled features [B, C_last].  T <= 32 gives exactly `cnn_pool`'s result; wider images run the
    32-wide conv kernels over overlapping column tiles (csrc/ww_cnn.hip, ColTiling)."""
    _require_x(x, MAX_FRAMES)
    _check_packed(packed, n_conv, x)
    return torch.ops.wakeword_amd.cnn_pool_wide(x, packed, n_conv)


def forward_pcm_frames(pcm, packed, n_conv, n_samples: int, normalize: bool = True):
    """pcm [B, n <= n_samples] -> logits [B, 2]: logmel_frames -> cnn_pool_wide -> lstm_fc in one native call."""
    _require_pcm(pcm, n_samples)
    _check_packed(packed, n_conv, pcm)
    return torch.ops.wakeword_amd.forward_pcm_frames(pcm, packed, n_conv, int(n_samples), bool(normalize))


# ------------------------------------------------------------------------------------------------
# training step (SimpleWakewordModel): train-mode forward + backward on the HIP kernels of csrc/ww_train.hip
# ------------------------------------------------------------------------------------------------
def _train_keys(n_conv):
    convs = [k for i in range(1, n_conv + 1) for k in (f"conv{i}.weight", f"conv{i}.bias")]
    return tuple(convs + ["lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0",
                          "lstm.weight_ih_l1", "lstm.weight_hh_l1", "lstm.bias_ih_l1", "lstm.bias_hh_l1", "fc.weight", "fc.bias"])


def _train_params_struct(params, n_conv):
    convs, (wi0, _wh0, bi0, bh0, wi1, _wh1, bi1, bh1, fw, fb) = params[:2 * n_conv], params[2 * n_conv:]
    tp = nat.TrainParams()
    tp.n_conv, tp.hidden = n_conv, 256
    for i in range(n_conv):
        tp.conv_weight[i], tp.conv_bias[i] = convs[2 * i].data_ptr(), convs[2 * i + 1].data_ptr()
    tp.lstm_weight_ih[0], tp.lstm_weight_ih[1] = wi0.data_ptr(), wi1.data_ptr()
    tp.lstm_bias_ih[0], tp.lstm_bias_ih[1] = bi0.data_ptr(), bi1.data_ptr()
    tp.lstm_bias_hh[0], tp.lstm_bias_hh[1] = bh0.data_ptr(), bh1.data_ptr()
    tp.fc_weight, tp.fc_bias = fw.data_ptr(), fb.data_ptr()
    return tp


def train_grads_struct(grads: dict, n_conv: int):
    """nat.TrainGrads over gradient tensors keyed by parameter name.  The struct has one bias gradient per LSTM layer, filed under
    bias_ih (d/d bias_hh is the same tensor), and none for weight_hh (h0 = 0 makes it exactly zero): those keys are not read."""
    tg = nat.TrainGrads()
    for i in range(n_conv):
        tg.conv_weight[i], tg.conv_bias[i] = grads[f"conv{i + 1}.weight"].data_ptr(), grads[f"conv{i + 1}.bias"].data_ptr()
    for layer in range(2):
        tg.lstm_weight_ih[layer], tg.lstm_bias[layer] = grads[f"lstm.weight_ih_l{layer}"].data_ptr(), grads[f"lstm.bias_ih_l{layer}"].data_ptr()
    tg.fc_weight, tg.fc_bias = grads["fc.weight"].data_ptr(), grads["fc.bias"].data_ptr()
    return tg


def train_workspace_bytes(B: int, n_conv: int, math: int) -> int:
    """ww_train_workspace_bytes; `math` is a resolved WW_TRAIN_MATH_* value (ww_get_train_math(), read ONCE per step and handed to the
    query, the forward and the backward alike)."""
    return nat.check(nat.lib.ww_train_workspace_bytes(B, n_conv, math))


def train_forward_into(x, tp, p_lstm, p_fc, seed, math, ws, logits) -> None:
    """ww_train_forward_f32 on checked arguments: x as _check_x returns it, `tp` from _train_params_struct, `ws` uint8 of at least
    train_workspace_bytes(B, n_conv, math), logits float32 [>= B, 2].  One native call on the current stream of the CURRENT device,
    which the caller has made x's (a guard per launch showed in the trainer's step at B = 16); allocates nothing."""
    nat.check(nat.lib.ww_train_forward_f32(_ptr(x), x.shape[0], x.shape[3], C.byref(tp), float(p_lstm), float(p_fc),
                                           int(seed) & (2 ** 64 - 1), math, _ptr(ws), ws.numel(), _ptr(logits), _stream()))


def train_backward_into(x, tp, dlogits, math, ws, tg) -> None:
    """ww_train_backward_f32 on the x, `tp`, `math` and `ws` of the forward it follows, dlogits float32 [>= B, 2] contiguous and `tg` from
    train_grads_struct.  One native call, x's device current as for train_forward_into; allocates nothing."""
    nat.check(nat.lib.ww_train_backward_f32(_ptr(x), x.shape[0], x.shape[3], C.byref(tp), _ptr(dlogits), math, _ptr(ws), ws.numel(),
                                            C.byref(tg), _stream()))


class _TrainStep(torch.autograd.Function):
    """logits = model(x) in train mode, with d loss / d parameters from the HIP backward kernels.  `x` gets no gradient (the
    reference never asks for one)."""
    # diagnostics only (train_last_masks / _packed_image / _bit_images): a WEAK reference to the newest step's workspace, so that it
    # does not outlive its step (a strong one kept 2.7 GB alive behind every fp32 step); tests that read it after the backward
    # switch keep_train_workspace(True) on
    _last_ws_ref = None
    _last_ws_keep = None
    keep = False
    last_n_conv = 2
    last_n = 0

    @staticmethod
    def forward(ctx, x, n_conv, p_lstm, p_fc, seed, *params):
        x = _check_x(x)
        params = tuple(p.detach().contiguous() for p in params)
        for p in params:
            _require_cuda_f32(p, "parameter")
        B = x.shape[0]
        if B == 0:
            raise ValueError("empty training batch")
        logits = torch.empty((B, 2), device=x.device, dtype=torch.float32)
        math = nat.lib.ww_get_train_math()                  # resolved ONCE: query, forward and backward of this step all get this value
        ws = torch.empty(train_workspace_bytes(B, n_conv, math), device=x.device, dtype=torch.uint8)
        with torch.cuda.device(x.device):
            train_forward_into(x, _train_params_struct(params, n_conv), p_lstm, p_fc, seed, math, ws, logits)
        ctx.save_for_backward(x, ws, *params)
        ctx.n_conv = n_conv
        ctx.train_math = math
        _TrainStep._last_ws_ref, _TrainStep.last_n_conv, _TrainStep.last_n = weakref.ref(ws), n_conv, B
        _TrainStep._last_ws_keep = ws if _TrainStep.keep else None
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        x, ws, *params = ctx.saved_tensors
        n_conv = ctx.n_conv
        dlogits = dlogits.contiguous().float()
        grads = {k: torch.empty_like(p) for k, p in zip(_train_keys(n_conv), params)}
        for layer in range(2):
            grads[f"lstm.weight_hh_l{layer}"].zero_()       # h0 = 0: the gradient is exactly zero
        with torch.cuda.device(x.device):
            train_backward_into(x, _train_params_struct(params, n_conv), dlogits, ctx.train_math, ws, train_grads_struct(grads, n_conv))
        for layer in range(2):
            grads[f"lstm.bias_hh_l{layer}"].copy_(grads[f"lstm.bias_ih_l{layer}"])       # d/d bias_hh == d/d bias_ih
        return (None, None, None, None, None, *grads.values())


def train_forward(x, named_params: dict, n_conv: int, p_lstm: float, p_fc: float, seed: int):
    """x [B,1,80,T] + the module's parameters (reference key set) -> logits [B,2] with an autograd graph behind them."""
    return _TrainStep.apply(x, n_conv, p_lstm, p_fc, seed, *[named_params[k] for k in _train_keys(n_conv)])


def keep_train_workspace(on: bool = True) -> None:
    """Diagnostics switch: hold a strong reference to the newest training step's workspace so that train_last_* can read it after
    the step's autograd graph is gone (off by default: the workspace then dies with its step)."""
    _TrainStep.keep = bool(on)
    if not on:
        _TrainStep._last_ws_keep = None


def _last_workspace() -> torch.Tensor:
    ws = _TrainStep._last_ws_ref() if _TrainStep._last_ws_ref is not None else None
    if ws is None:
        raise RuntimeError("no live training workspace: the last step's graph was freed (ops.keep_train_workspace(True) keeps it for diagnostics)")
    return ws


def train_last_masks(n: int):
    """Dropout factors of the most recent training forward: (mask0 [n,256], mask1 [n,256]) -- tests replay them elsewhere."""
    ws = _last_workspace()
    m0 = torch.empty((n, 256), device=ws.device, dtype=torch.float32)
    m1 = torch.empty_like(m0)
    with torch.cuda.device(ws.device):
        nat.check(nat.lib.ww_train_masks(_ptr(ws), n, _TrainStep.last_n_conv, _ptr(m0), _ptr(m1), _stream()))
    return m0, m1


_TRAIN_STAGES = ("pooled", "gates0", "gates1", "hd0", "hd1", "dhd1", "dg1", "dhd0", "dg0", "dpooled", "gp", "dz2", "mid2", "mid3")   # WW_TRAIN_STAGE_*


def train_stages(train_math: str, names=None) -> dict:
    """Diagnostic, read-only: the intermediates of the newest kept training workspace, {name: float32 tensor}.
      pooled [n,C]; gates0/1 [4,n,256] (planes sigmoid i, tanh g, sigmoid o, tanh c); hd0/1 [n,256]   -- written by the forward
      dhd1, dhd0 [n,256]; dg1, dg0 [n,1024] (torch's i,f,g,o rows); dpooled, gp [n,C]                  -- written by the backward
      3-conv model: dz2 [n,64,80,32] (backward; split mode: decoded, per-clip scales applied)
      mid2 [n,64,80,32] / mid3 [n,128,80,32] where the arithmetic keeps them (forward)
    `train_math` must name the arithmetic the step ran under: the library refuses a workspace it has no forward on record for
    or whose forward ran under the other one, and the backward's stages until the backward has run.
    `names` restricts the copy to some stages (mid2 is 2.7 GB at 4096 clips)."""
    if train_math not in TRAIN_MATH:
        raise ValueError(f"train math {train_math!r}: expected one of {sorted(TRAIN_MATH)}")
    ws, n, nc = _last_workspace(), _TrainStep.last_n, _TrainStep.last_n_conv
    C_last, split = c_last(nc), train_math == "f16x3"
    shapes = {"pooled": (n, C_last), "gates0": (4, n, 256), "gates1": (4, n, 256), "hd0": (n, 256), "hd1": (n, 256), "dhd1": (n, 256),
              "dg1": (n, 1024), "dhd0": (n, 256), "dg0": (n, 1024), "dpooled": (n, C_last), "gp": (n, C_last)}
    if nc == 3:
        shapes["dz2"] = (n, 80, 64, 32)
    if nc == 3 or not split:
        shapes["mid2"] = (n, 80, 64, 32)
    if nc == 3 and not split:
        shapes["mid3"] = (n, 80, 128, 32)
    out = {}
    with torch.cuda.device(ws.device):
        for name, shape in shapes.items():
            if names is not None and name not in names:
                continue
            t = torch.empty(shape, device=ws.device, dtype=torch.float32)
            nat.check(nat.lib.ww_train_stage(_ptr(ws), n, nc, TRAIN_MATH[train_math], _TRAIN_STAGES.index(name), _ptr(t), t.numel(), _stream()))
            out[name] = t.permute(0, 2, 1, 3) if len(shape) == 4 else t          # [n, C, 80, 32] view
    return out


def train_last_packed_image() -> torch.Tensor:
    """Diagnostic: the packed image the most recent split-precision training forward of the 2-conv model wrote on the device."""
    ws = _last_workspace()
    img = torch.empty(int(nat.lib.ww_packed_weights_floats(_TrainStep.last_n_conv)), device=ws.device, dtype=torch.float32)
    with torch.cuda.device(ws.device):
        nat.check(nat.lib.ww_train_packed_image(_ptr(ws), _TrainStep.last_n, _TrainStep.last_n_conv, _ptr(img), _stream()))
    return img


def train_last_bit_images():
    """Diagnostic: (mask_last uint8 [n,80,32,C/8], sign1 int32 [n,80,32]) of the most recent split-precision training forward."""
    ws, n, nc = _last_workspace(), _TrainStep.last_n, _TrainStep.last_n_conv
    mask = torch.empty((n, 80, 32, 8 if nc == 2 else 16), device=ws.device, dtype=torch.uint8)
    sign1 = torch.empty((n, 80, 32), device=ws.device, dtype=torch.int32)
    with torch.cuda.device(ws.device):
        nat.check(nat.lib.ww_train_bit_images(_ptr(ws), n, nc, _ptr(mask), _ptr(sign1), _stream()))
    return mask, sign1


CONV_MATH = {"f32": 0, "f16x3": 1, "f16x3d": 2}
LOGMEL_MATH = {"f32": 0, "f64": 1, "auto": 2}
TRAIN_MATH = {"f32": 0, "f16x3": 1}
_MATH = {"conv": ("conv math", CONV_MATH), "logmel": ("log-mel math", LOGMEL_MATH), "train": ("train math", TRAIN_MATH)}   # ww_{set,get}_<kind>_math


def _set_math(kind: str, mode, thread: bool = False) -> None:
    what, table = _MATH[kind]
    if mode not in table and not (thread and mode is None):
        raise ValueError(f"{what} {mode!r}: expected one of {sorted(table)}" + (" or None" if thread else ""))
    nat.check(getattr(nat.lib, f"ww_set_{kind}_math" + ("_thread" if thread else ""))(-1 if mode is None else table[mode]))


def _get_math(kind: str) -> str:
    return {v: k for k, v in _MATH[kind][1].items()}[getattr(nat.lib, f"ww_get_{kind}_math")()]


def set_conv_math(mode: str) -> None:
    """Arithmetic of the conv / LSTM-gate GEMMs, process-wide: 'f32' (exact fp32 MFMA), 'f16x3' (each fp32 operand as two f16
    halves, three f16 MFMAs per product block, fp32 accumulate; ~2^-21 relative error, 3/16 the MFMA cycles; the 2-conv model's
    conv2 as a 1-D Winograd F(2,3)) or 'f16x3d' (f16x3 with every convolution in its direct form)."""
    _set_math("conv", mode)


def set_conv_math_thread(mode) -> None:
    """Override the conv arithmetic for launches issued by the CALLING THREAD only (None clears it): a streamer thread and a batch
    job can then use different arithmetics safely."""
    _set_math("conv", mode, thread=True)


def get_conv_math() -> str:
    return _get_math("conv")


def set_logmel_math(mode: str) -> None:
    """Arithmetic of the log-mel front end, process-wide: 'f32' (float32 FFT), 'f64' (float64 window product / FFT / split, what
    the reference's numpy.fft.rfft computes) or 'auto' (default: float32, and the clips with a live mel band on the float32
    FFT's rounding floor are redone in float64)."""
    _set_math("logmel", mode)


def set_logmel_math_thread(mode) -> None:
    """Per-thread override of the log-mel arithmetic (None clears it); see set_conv_math_thread."""
    _set_math("logmel", mode, thread=True)


def get_logmel_math() -> str:
    return _get_math("logmel")


def set_train_math(mode: str) -> None:
    """Arithmetic of the training step's conv kernels, process-wide: 'f16x3' (default: split precision on the f16 matrix
    instructions where a kernel exists -- SimpleWakewordModel's conv2 backward) or 'f32' (exact fp32 matrix instructions)."""
    _set_math("train", mode)


def get_train_math() -> str:
    return _get_math("train")


def init() -> None:
    """Upload the front-end tables for the current device (needed before hipGraph capture)."""
    nat.check(nat.lib.ww_init())


if os.environ.get("WW_CONV_MATH"):
    set_conv_math(os.environ["WW_CONV_MATH"])
if os.environ.get("WW_LOGMEL_MATH"):
    set_logmel_math(os.environ["WW_LOGMEL_MATH"])


# ---- KA: augmentation ------------------------------------------------------------------
AUG_MAX_SAMPLES = 16383                 # T = 1 + N // 512 <= 32 frames: the clip lengths training takes (4000 .. 16383 samples)


def _require_clips(pcm, name: str, max_samples: int, min_rows: int = 0) -> None:
    """pcm float32 [B >= min_rows, N] on the GPU, N in MIN_CLIP_SAMPLES..max_samples: what `name`, an augmentation function, takes."""
    if pcm.device.type != "cuda":
        raise RuntimeError(f"{name}: pcm must live on the MI355X (no CPU fallback)")
    if pcm.dtype != torch.float32 or pcm.dim() != 2 or not MIN_CLIP_SAMPLES <= pcm.shape[1] <= max_samples or pcm.shape[0] < min_rows:
        raise ValueError(f"{name}: expected float32 [{'B' if min_rows == 0 else f'B >= {min_rows}'}, N], N in {MIN_CLIP_SAMPLES}..{max_samples}, "
                         f"got {pcm.dtype} {tuple(pcm.shape)}")


def _plans_array(plans, B):
    """A ctypes array of _native.AugmentPlan as it is, a list of dict plans converted to one."""
    if isinstance(plans, C.Array):
        if len(plans) < B:
            raise ValueError(f"augment: {len(plans)} plans for {B} clips")
        return plans
    arr = (nat.AugmentPlan * max(1, B))()
    if len(plans) != B:
        raise ValueError(f"augment: {len(plans)} plans for {B} clips")
    for i, p in enumerate(plans):
        a = arr[i]
        a.shift = int(p.get("shift", 0))
        a.crop_start = int(p.get("crop", 0))
        n_steps = p.get("n_steps")
        a.pitch_rate = float(p["pitch_rate"]) if p.get("pitch_rate") else (2.0 ** (-float(n_steps) / 12.0) if n_steps is not None else 0.0)
        a.stretch_rate = float(p["rate"]) if p.get("rate") else 0.0
        a.noise_sigma = float(p.get("sigma", 0.0))
        a.noise_seed = int(p.get("seed", 0)) & 0xFFFFFFFF
    return arr


def augment(pcm: torch.Tensor, plans, bank=None, rirs=None) -> torch.Tensor:
    """pcm [B, N] float32 on the GPU + one plan per clip -> augmented [B, N], N in 4000..16383 (ww_augment_rir_f32 for every batch; the
    plans' shift is taken mod N and crop lies in [0, round(N / rate) - N]).

    `plans`: a ctypes array of _native.AugmentPlan, or a list of dicts with the keys of oracle-style plans
    (shift, n_steps | pitch_rate, rate, crop, sigma, seed); see AudioProcessor.draw_augment_plan.
    With a background.BackgroundNoiseBank, dict plans that carry `bg_file`, `bg_start` and `snr_db` get that file's segment mixed in after
    the stretch and before the Gaussian noise; clips without those keys, and a batch where no plan has them, give
    exactly what they give without a bank.
    With a reverb.ImpulseResponseBank (`rirs`), dict plans that carry `rir` get that room impulse response after the stretch and before
    the background; clips without the key, and a batch where no plan has it, give exactly what they give without."""
    _require_clips(pcm, "augment", AUG_MAX_SAMPLES)
    N = int(pcm.shape[1])
    pcm = pcm.contiguous() if N == CLIP_SAMPLES else _aligned_rows(pcm)
    B = pcm.shape[0]
    bg_plans = rir_plans = None
    if not isinstance(plans, C.Array):
        if bank is not None and any("bg_file" in p for p in plans):
            bg_plans = plans
        if rirs is not None and any(p.get("rir") is not None for p in plans):
            rir_plans = plans
    plans = _plans_array(plans, B)
    bg = _bg_array(bg_plans, bank, B) if bg_plans else None
    rir = _rir_array(rir_plans or (), rirs, B)
    out = torch.empty((B, N), device=pcm.device, dtype=torch.float32)
    if B == 0:
        return out
    # one native call for every batch: without background bg is NULL, without reverb every rir entry is off, and a stage that no clip
    # uses is neither copied nor launched
    bank_ptr = spectra_ptr = None
    bank_len = n_rirs = 0
    if rir_plans:
        _check_rirs(rirs, pcm.device)
        spectra_ptr, n_rirs = C.c_void_p(rirs.spectra.data_ptr()), rirs.n_rirs
    if bg is not None:
        _check_bank(bank, pcm.device)
        bank_ptr, bank_len = C.c_void_p(bank.data.data_ptr()), bank.data.numel()
    with torch.cuda.device(pcm.device):
        ws = torch.empty(nat.check(nat.lib.ww_augment_rir_workspace_bytes(B, N)), device=pcm.device, dtype=torch.uint8)
        nat.check(nat.lib.ww_augment_rir_f32(C.c_void_p(pcm.data_ptr()), B, pcm.stride(0) if B > 1 else N, N, plans, bg, bank_ptr, bank_len,
                                             rir, spectra_ptr, n_rirs, C.c_void_p(out.data_ptr()), N, C.c_void_p(ws.data_ptr()),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        ws.record_stream(torch.cuda.current_stream())
    return out


# the per-clip record of csrc/ww_augment.hip (AugDev), ww_augment_record_bytes() bytes each
AUG_RECORD_DTYPE = [("shift", "<i4"), ("crop", "<i4"), ("p_out", "<i4"), ("p_len", "<i4"), ("p_res", "<i4"), ("s_out", "<i4"),
                    ("s_len", "<i4"), ("seed", "<u4"), ("p_rate", "<f8"), ("p_ratio", "<f8"), ("s_rate", "<f8"), ("sigma", "<f4"), ("pad", "<f4")]


def augment_stages(pcm: torch.Tensor, plans, poison: bool = False) -> dict:
    """Diagnostic: ops.augment(pcm, plans) with the kernel chain's intermediates, viewed from the workspace of this call through
    ww_augment_workspace_layout and cut to each clip's real sizes.  One vocoder pass only: a batch whose plans turn on both pitch and
    stretch is refused (the second pass overwrites S), and so are background and reverb keys.  Returns
        "records"  numpy structured array [B] (AUG_RECORD_DTYPE): what the kernels read for each clip
        "rolled"   [B, row] the work buffer the STFT reads: np.roll of the input, rows padded with zeros to four floats
        "S"        list of complex64 [steps, 1025]: the vocoder's output columns (steps = p_out or s_out; 0 rows for a clip with the pass off)
        "Y"        list of float32 [p_len]: the pitch pass's inverse STFT before resampling (empty for stretch batches and pitch-off clips)
        "Y_tail"   list of float32 [4]: the four floats past Y (never written; with `poison` they stay NaN)
        "stage"    [B, row] the chain's last work buffer: the resampled clips (pitch batch), the cropped / zero-padded inverse STFT
                   (stretch batch), the rolled input (neither)
        "out"      [B, N] the call's result (the stage plus the plans' Gaussian noise)
    `poison` fills the workspace with float32 NaN before the call: whatever a kernel reads without having written it shows in the output."""
    _require_clips(pcm, "augment_stages", AUG_MAX_SAMPLES, min_rows=1)
    if not isinstance(plans, C.Array) and any(k in p for p in plans for k in ("bg_file", "rir")):
        raise ValueError("augment_stages: background and reverb are not staged")
    N = int(pcm.shape[1])
    pcm = pcm.contiguous() if N == CLIP_SAMPLES else _aligned_rows(pcm)
    B = pcm.shape[0]
    plans = _plans_array(plans, B)
    any_pitch = any(plans[i].pitch_rate != 0.0 for i in range(B))
    any_stretch = any(plans[i].stretch_rate != 0.0 for i in range(B))
    if any_pitch and any_stretch:
        raise ValueError("augment_stages: the batch turns on both pitch and stretch; the stretch pass overwrites the pitch pass's S")
    lay = nat.AugmentLayout()
    nat.check(nat.lib.ww_augment_workspace_layout(B, N, C.byref(lay)))
    out = torch.empty((B, N), device=pcm.device, dtype=torch.float32)
    with torch.cuda.device(pcm.device):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ws = torch.empty(lay.total_bytes, device=pcm.device, dtype=torch.uint8)
        if poison:
            ws.view(torch.float32).fill_(float("nan"))
        assert lay.total_bytes == nat.check(nat.lib.ww_augment_n_workspace_bytes(B, N))
        nat.check(nat.lib.ww_augment_n_f32(C.c_void_p(pcm.data_ptr()), B, pcm.stride(0) if B > 1 else N, N, plans,
                                           C.c_void_p(out.data_ptr()), N, C.c_void_p(ws.data_ptr()), stream))
        torch.cuda.current_stream().synchronize()

    def region(off, stride, dtype=torch.float32):
        return ws[off:off + B * stride].view(dtype).view(B, -1)
    rec = np.frombuffer(ws[lay.records:lay.records + B * lay.record_bytes].cpu().numpy().tobytes(), dtype=np.dtype(AUG_RECORD_DTYPE))
    assert rec.itemsize == lay.record_bytes
    buf_a, buf_b = region(lay.buf_a, lay.row_bytes), region(lay.buf_b, lay.row_bytes)
    spec = torch.view_as_complex(region(lay.spec, lay.spec_clip_bytes).view(B, -1, lay.spec_step_bytes // 8, 2))
    y = region(lay.y, lay.y_clip_bytes)
    steps = [int(r["p_out"] if any_pitch else r["s_out"]) for r in rec]
    return {"records": rec, "rolled": buf_a, "S": [spec[i, :steps[i]] for i in range(B)],
            "Y": [y[i, :int(rec[i]["p_len"]) if rec[i]["p_out"] else 0] for i in range(B)],
            "Y_tail": [y[i, int(rec[i]["p_len"]):int(rec[i]["p_len"]) + 4] for i in range(B)],
            "stage": buf_b if (any_pitch or any_stretch) else buf_a, "out": out}


def _check_bank(bank, device) -> None:
    data = getattr(bank, "data", None)
    if not isinstance(data, torch.Tensor) or data.dtype != torch.float32 or data.dim() != 1:
        raise TypeError("bank: expected a background.BackgroundNoiseBank")
    if data.device != device:
        raise ValueError(f"bank: lives on {data.device}, the clips on {device}")


def _bg_array(plans, bank, B):
    """Plans (dicts with bg_file / bg_start / snr_db, or without them: no background) -> ctypes array of _native.AugmentBg."""
    bg = (nat.AugmentBg * max(1, B))()
    for i, p in enumerate(plans):
        if p.get("bg_file") is None:
            continue
        f = int(p["bg_file"])
        if not 0 <= f < bank.n_files:
            raise ValueError(f"bg_file {f}: the bank holds {bank.n_files} files")
        b = bg[i]
        b.file_offset, b.file_len = int(bank.offsets[f]), int(bank.lengths[f])
        b.start, b.snr_db, b.enabled = int(p.get("bg_start", 0)), float(p["snr_db"]), 1
    return bg


def mix_background(pcm: torch.Tensor, bank, files, starts, snr_db) -> torch.Tensor:
    """The background mix alone (ww_mix_background_f32): pcm [B, N] float32 on the GPU, N in 4000..32000 (every inference length) ->
    [B, N] with clip i + bank file `files[i]` from sample `starts[i]` (wrapping around the file) at `snr_db[i]` dB (a scalar applies to
    every clip).  A negative file index leaves that clip as it is.  For noisy evaluation sets at a fixed SNR."""
    _require_clips(pcm, "mix_background", MAX_CLIP_SAMPLES)
    _check_bank(bank, pcm.device)
    B, N = int(pcm.shape[0]), int(pcm.shape[1])
    if pcm.stride(1) != 1:
        pcm = pcm.contiguous()
    files, starts = np.broadcast_to(np.asarray(files, dtype=np.int64), (B,)), np.broadcast_to(np.asarray(starts, dtype=np.int64), (B,))
    snr = np.broadcast_to(np.asarray(snr_db, dtype=np.float64), (B,))
    plans = [{} if files[i] < 0 else {"bg_file": int(files[i]), "bg_start": int(starts[i]), "snr_db": float(snr[i])} for i in range(B)]
    bg = _bg_array(plans, bank, B)
    out = torch.empty((B, N), device=pcm.device, dtype=torch.float32)
    if B == 0:
        return out
    with torch.cuda.device(pcm.device):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ws = torch.empty(nat.check(nat.lib.ww_mix_background_workspace_bytes(B)), device=pcm.device, dtype=torch.uint8)
        nat.check(nat.lib.ww_mix_background_f32(C.c_void_p(pcm.data_ptr()), B, pcm.stride(0) if B > 1 else N, N, bg,
                                                C.c_void_p(bank.data.data_ptr()), bank.data.numel(), C.c_void_p(out.data_ptr()), N,
                                                C.c_void_p(ws.data_ptr()), stream))
        ws.record_stream(torch.cuda.current_stream())
    return out


def _check_rirs(rirs, device) -> None:
    spectra = getattr(rirs, "spectra", None)
    if not isinstance(spectra, torch.Tensor) or spectra.dtype != torch.float32 or spectra.dim() != 3 or not spectra.is_contiguous():
        raise TypeError("rirs: expected a reverb.ImpulseResponseBank")
    if spectra.device != device:
        raise ValueError(f"rirs: lives on {spectra.device}, the clips on {device}")


def _rir_array(plans, rirs, B):
    """Plans (dicts with `rir`, or without it: no reverb) -> ctypes array of _native.AugmentRir."""
    arr = (nat.AugmentRir * max(1, B))()
    for i, p in enumerate(plans):
        r = p.get("rir")
        if r is None:
            continue
        r = int(r)
        if not 0 <= r < rirs.n_rirs:
            raise ValueError(f"rir {r}: the bank holds {rirs.n_rirs} impulse responses")
        a = arr[i]
        a.index, a.dpos, a.taps, a.enabled = r, int(rirs.dpos[r]), int(rirs.lengths[r]), 1
    return arr


def reverb(pcm: torch.Tensor, rirs, index) -> torch.Tensor:
    """The reverb alone (ww_reverb_f32): pcm [B, N] float32 on the GPU, N in 4000..32000 (every inference length) -> [B, N] with clip i
    convolved with bank RIR `index[i]` (a scalar applies to every clip), advanced by its direct-path delay and rescaled to the clip's
    energy.  A negative index leaves that clip as it is.  For reverberant evaluation sets."""
    _require_clips(pcm, "reverb", MAX_CLIP_SAMPLES)
    _check_rirs(rirs, pcm.device)
    B, N = int(pcm.shape[0]), int(pcm.shape[1])
    if pcm.stride(1) != 1:
        pcm = pcm.contiguous()
    idx = np.broadcast_to(np.asarray(index, dtype=np.int64), (B,))
    rir = _rir_array([{} if idx[i] < 0 else {"rir": int(idx[i])} for i in range(B)], rirs, B)
    out = torch.empty((B, N), device=pcm.device, dtype=torch.float32)
    if B == 0:
        return out
    with torch.cuda.device(pcm.device):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ws = torch.empty(nat.check(nat.lib.ww_reverb_workspace_bytes(B)), device=pcm.device, dtype=torch.uint8)
        nat.check(nat.lib.ww_reverb_f32(C.c_void_p(pcm.data_ptr()), B, pcm.stride(0) if B > 1 else N, N, rir,
                                        C.c_void_p(rirs.spectra.data_ptr()), rirs.n_rirs, C.c_void_p(out.data_ptr()), N,
                                        C.c_void_p(ws.data_ptr()), stream))
        ws.record_stream(torch.cuda.current_stream())
    return out


# ---- loss, metrics and optimiser of the training loop (csrc/ww_optim.hip) ---------------------------------
LOSS_STATS_FIELDS = ("loss_sum", "correct", "total", "batches", "bad_labels", "nonfinite")


def new_loss_stats(device) -> torch.Tensor:
    """A zeroed ww_loss_stats record in device memory: six 8-byte words (the first a float64); `stats.zero_()` starts a new epoch."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"loss stats on {device}: this path has no CPU implementation")
    return torch.zeros(len(LOSS_STATS_FIELDS), device=device, dtype=torch.int64)


def _check_stats(stats, like: torch.Tensor) -> None:
    if (not isinstance(stats, torch.Tensor) or stats.dtype != torch.int64 or stats.shape != (len(LOSS_STATS_FIELDS),)
            or not stats.is_contiguous()):
        raise TypeError("stats: expected the record ops.new_loss_stats() makes (int64 [6], contiguous)")
    if stats.device != like.device:
        raise RuntimeError(f"stats on {stats.device}, logits on {like.device}")


def read_loss_stats(stats: torch.Tensor) -> dict:
    """The record on the host: {loss_sum: float, correct, total, batches, bad_labels, nonfinite: int}.  One device-to-host copy."""
    host = stats.cpu()
    out = {k: int(v) for k, v in zip(LOSS_STATS_FIELDS[1:], host[1:].tolist())}
    out["loss_sum"] = float(host[:1].view(torch.float64).item())
    return out


def _check_logits(logits) -> None:
    _require_cuda_f32(logits, "logits")
    if logits.dim() != 2 or logits.shape[1] != 2 or logits.shape[0] == 0 or not logits.is_contiguous():
        raise ValueError(f"logits: expected contiguous [n >= 1, 2], got {tuple(logits.shape)}")


def _check_ce(logits, labels):
    _check_logits(logits)
    if not isinstance(labels, torch.Tensor):
        raise TypeError(f"labels: expected a torch.Tensor, got {type(labels).__name__}")
    if labels.dtype != torch.int64:
        raise TypeError(f"labels: expected int64, got {labels.dtype}")
    if labels.device != logits.device:
        raise RuntimeError(f"labels on {labels.device}, logits on {logits.device}")
    if labels.dim() == 2 and labels.shape[1] == 1:
        labels = labels[:, 0]                                # the reference squeezes [B, 1] targets
    if labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
        raise ValueError(f"labels: expected [{logits.shape[0]}] or [{logits.shape[0]}, 1], got {tuple(labels.shape)}")
    return labels if labels.stride(0) == 1 or labels.shape[0] == 1 else labels.contiguous()


def loss_opts(weight=None, label_smoothing=0.0, ignore_index=-100, reduction="mean", focal_gamma=None):
    """The loss options as the struct ww_ce_loss_ex_f32 takes (nat.LossOpts, host memory), or None when every option is at its default:
    the plain ww_ce_loss_f32 call.  ValueError / NotImplementedError (reduction="none") before any device call (loss.check_options)."""
    from .loss import check_options
    w, eps, ignore, reduction, gamma = check_options(weight, label_smoothing, ignore_index, reduction, focal_gamma)
    if w is None and eps == 0.0 and ignore == -100 and reduction == "mean" and gamma is None:
        return None
    o = nat.LossOpts()
    o.class_weight[0], o.class_weight[1] = w if w is not None else (1.0, 1.0)
    o.label_smoothing, o.focal_gamma, o.ignore_index = eps, 0.0 if gamma is None else gamma, ignore
    o.kind = nat.LOSS_CE if gamma is None else nat.LOSS_FOCAL
    o.reduction = nat.REDUCE_MEAN if reduction == "mean" else nat.REDUCE_SUM
    return o


def _loss_launch(logits, targets, soft: bool, opts, dlogits, loss, stats) -> None:
    """ww_ce_loss_soft_f32 on class probabilities (`soft`), else ww_ce_loss_f32 without options and ww_ce_loss_ex_f32 with them."""
    fn = nat.lib.ww_ce_loss_soft_f32 if soft else nat.lib.ww_ce_loss_f32 if opts is None else nat.lib.ww_ce_loss_ex_f32
    byref = () if opts is None and not soft else (None if opts is None else C.byref(opts),)      # soft: NULL options are the defaults
    with torch.cuda.device(logits.device):
        nat.check(fn(_ptr(logits), _ptr(targets), logits.shape[0], *byref, None if dlogits is None else _ptr(dlogits),
                     None if loss is None else _ptr(loss), None if stats is None else _ptr(stats), _stream()))


def _loss_alloc_launch(logits, targets, soft: bool, opts, stats, grad: bool):
    """The tail of ce_loss and soft_ce_loss on checked inputs: check the stats record, allocate loss and dlogits, launch."""
    if stats is not None:
        _check_stats(stats, logits)
    loss, dlogits = torch.empty((), device=logits.device, dtype=torch.float32), torch.empty_like(logits) if grad else None
    _loss_launch(logits, targets, soft, opts, dlogits, loss, stats)
    return loss, dlogits


def ce_loss_into(logits, labels, dlogits, loss, stats, *, weight=None, label_smoothing=0.0, ignore_index=-100, reduction="mean",
                 focal_gamma=None, opts=None) -> None:
    """ww_ce_loss_f32 -- or, with any loss option given, ww_ce_loss_ex_f32 -- on caller-owned outputs (each may be None); `labels` as
    _check_ce returns them.  `opts`: what ops.loss_opts() made of the options, built once by a caller that launches per batch (it wins
    over the keywords).  Allocates nothing on the device."""
    opts = loss_opts(weight, label_smoothing, ignore_index, reduction, focal_gamma) if opts is None else opts
    _loss_launch(logits, labels, False, opts, dlogits, loss, stats)


def ce_loss(logits: torch.Tensor, labels: torch.Tensor, stats=None, grad: bool = True, *, weight=None, label_smoothing=0.0,
            ignore_index=-100, reduction="mean", focal_gamma=None):
    """CrossEntropyLoss (mean) over two classes: (loss [] float32, dlogits [n, 2] = (softmax - onehot) / n, or None with grad=False).
    logits [n, 2] float32 and labels [n] or [n, 1] int64 on the GPU.  `stats` (ops.new_loss_stats) accumulates the batch mean, the correct
    predictions and the counts of bad labels and non-finite logits on the device; nothing here waits for it.

    The keyword-only options are those of F.cross_entropy: `weight` (two floats or a tensor of two),
    `label_smoothing`, `ignore_index`, `reduction` ("mean" or "sum"; "none" raises NotImplementedError); `focal_gamma` (a number) turns
    the loss into the focal loss of loss.FocalLoss.  A bad value raises ValueError before any device call.  With every option at its
    default this is the ww_ce_loss_f32 call it always was, and a label of -100 is then a BAD label like any other outside {0, 1}; as soon
    as one option differs from its default, labels equal to `ignore_index` (-100 unless said otherwise) are ignored as torch ignores
    them.  When the mean's denominator is 0 the loss is NaN, as in torch, and the gradient is all zeros, unlike torch's."""
    opts = loss_opts(weight, label_smoothing, ignore_index, reduction, focal_gamma)
    return _loss_alloc_launch(logits, _check_ce(logits, labels), False, opts, stats, grad)


# ---- class-probability targets: soft cross-entropy and mixup (csrc/ww_optim.hip, csrc/ww_mixup.hip) --------
def _check_soft(logits, targets):
    _check_logits(logits)
    if not isinstance(targets, torch.Tensor):
        raise TypeError(f"targets: expected a torch.Tensor, got {type(targets).__name__}")
    if targets.dtype != torch.float32:
        raise TypeError(f"targets: expected float32 class probabilities, got {targets.dtype} (integer labels go to ops.ce_loss)")
    if targets.device != logits.device:
        raise RuntimeError(f"targets on {targets.device}, logits on {logits.device}")
    if targets.shape != logits.shape or not targets.is_contiguous():
        raise ValueError(f"targets: expected contiguous [{logits.shape[0]}, 2], got {tuple(targets.shape)}")


def soft_loss_opts(weight=None, label_smoothing=0.0, reduction="mean", focal_gamma=None, ignore_index=-100):
    """The options of ops.soft_ce_loss as the struct ww_ce_loss_soft_f32 takes, or None when every option is at its default.
    NotImplementedError for a focal loss or reduction="none", ValueError for an ignore_index other than -100 (torch refuses one for
    floating-point targets) and for every value ops.loss_opts refuses; nothing touches a device except a weight tensor's copy."""
    if focal_gamma is not None:
        raise NotImplementedError("soft_ce_loss: the focal loss takes integer labels (ops.ce_loss); class-probability targets take cross-entropy")
    opts = loss_opts(weight, label_smoothing, ignore_index, reduction, None)
    if int(ignore_index) != -100:
        raise ValueError(f"ignore_index {ignore_index}: class-probability targets take none (torch refuses it too)")
    return opts


def soft_ce_loss_into(logits, targets, dlogits, loss, stats, *, weight=None, label_smoothing=0.0, reduction="mean", focal_gamma=None,
                      opts=None) -> None:
    """ww_ce_loss_soft_f32 on caller-owned outputs (each may be None); `opts` as in ce_loss_into (what soft_loss_opts made; it wins
    over the keywords).  Allocates nothing on the device."""
    opts = soft_loss_opts(weight, label_smoothing, reduction, focal_gamma) if opts is None else opts
    _loss_launch(logits, targets, True, opts, dlogits, loss, stats)


def soft_ce_loss(logits: torch.Tensor, targets: torch.Tensor, stats=None, grad: bool = True, *, weight=None, label_smoothing=0.0,
                 reduction="mean", focal_gamma=None):
    """F.cross_entropy(logits, targets, weight=, label_smoothing=, reduction=) with class PROBABILITIES as targets: (loss [] float32,
    dlogits [n, 2] or None with grad=False).  logits and targets float32 contiguous [n, 2] on the GPU; `stats` as in ce_loss.  A target
    row counts iff both entries are finite and >= 0 (ops.mixup marks a row it could not label with NaN): any other row adds nothing, gets
    a zero gradient and is counted in bad_labels.  "mean" divides by the NUMBER of counted rows, as torch divides by n -- not by the
    weighted denominator of ce_loss.  With one-hot targets and default options the results have ce_loss's
    bits.  `focal_gamma` and reduction="none" raise NotImplementedError."""
    opts = soft_loss_opts(weight, label_smoothing, reduction, focal_gamma)
    _check_soft(logits, targets)
    return _loss_alloc_launch(logits, targets, True, opts, stats, grad)


# ---- knowledge distillation: hard term + teacher term in one launch (csrc/ww_optim.hip) --------------------
DISTILL_STATS_FIELDS = ("hard_sum", "kd_sum", "kd_rows", "hard_rows", "agree", "teacher_correct", "teacher_nonfinite", "batches")


def new_distill_stats(device) -> torch.Tensor:
    """A zeroed ww_distill_stats record in device memory: eight 8-byte words (the first two float64); `.zero_()` starts a new epoch."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"distillation stats on {device}: this path has no CPU implementation")
    return torch.zeros(len(DISTILL_STATS_FIELDS), device=device, dtype=torch.int64)


def _check_distill_stats(stats, like: torch.Tensor) -> None:
    if (not isinstance(stats, torch.Tensor) or stats.dtype != torch.int64 or stats.shape != (len(DISTILL_STATS_FIELDS),)
            or not stats.is_contiguous()):
        raise TypeError("distill_stats: expected the record ops.new_distill_stats() makes (int64 [8], contiguous)")
    if stats.device != like.device:
        raise RuntimeError(f"distill_stats on {stats.device}, logits on {like.device}")


def read_distill_stats(stats: torch.Tensor) -> dict:
    """The record on the host: {hard_sum, kd_sum: float, kd_rows, hard_rows, agree, teacher_correct, teacher_nonfinite, batches: int}.
    One device-to-host copy (none for a record that already is on the host)."""
    host = stats.cpu()
    out = {k: int(v) for k, v in zip(DISTILL_STATS_FIELDS[2:], host[2:].tolist())}
    out["hard_sum"], out["kd_sum"] = (float(v) for v in host[:2].view(torch.float64).tolist())
    return out


def _check_teacher_logits(logits, teacher_logits) -> None:
    if not isinstance(teacher_logits, torch.Tensor):
        raise TypeError(f"teacher_logits: expected a torch.Tensor, got {type(teacher_logits).__name__}")
    if teacher_logits.dtype != torch.float32:
        raise TypeError(f"teacher_logits: expected float32, got {teacher_logits.dtype}")
    if teacher_logits.device != logits.device:
        raise RuntimeError(f"teacher_logits on {teacher_logits.device}, logits on {logits.device}")
    if teacher_logits.shape != logits.shape or not teacher_logits.is_contiguous():
        raise ValueError(f"teacher_logits: expected contiguous [{logits.shape[0]}, 2], got {tuple(teacher_logits.shape)}")


def distill_opts(targets, weight=None, label_smoothing=0.0, ignore_index=-100, reduction="mean", focal_gamma=None):
    """The hard term's options for the kind of `targets` (None, int64 labels, float32 probabilities), as ww_distill_loss_f32 takes them,
    or None when every option is at its default.  Without a target only `reduction` is kept; refusals as loss_opts / soft_loss_opts."""
    if targets is None:
        loss_opts(weight, label_smoothing, ignore_index, reduction, focal_gamma)           # checked, then all but the reduction dropped
        return loss_opts(reduction=reduction)
    if targets.dtype == torch.float32:
        return soft_loss_opts(weight, label_smoothing, reduction, focal_gamma, ignore_index)
    return loss_opts(weight, label_smoothing, ignore_index, reduction, focal_gamma)


def distill_loss_into(logits, teacher_logits, targets, dlogits, loss, stats, distill_stats, *, alpha=0.5, temperature=2.0, weight=None,
                      label_smoothing=0.0, ignore_index=-100, reduction="mean", focal_gamma=None, opts=None) -> None:
    """ww_distill_loss_f32 on caller-owned outputs (each may be None) and checked inputs: `targets` None (no target), int64 labels as
    _check_ce returns them, or float32 probabilities [n, 2].  `opts`: what distill_opts made of the options, built once by a caller that
    launches per batch (it wins over the keywords).  alpha and temperature are checked on the host (loss.check_distillation) before
    anything is launched.  Allocates nothing on the device."""
    from .loss import check_distillation
    alpha, temperature = check_distillation(alpha, temperature)
    opts = distill_opts(targets, weight, label_smoothing, ignore_index, reduction, focal_gamma) if opts is None else opts
    kind = nat.TARGET_PROBS if targets is not None and targets.dtype == torch.float32 else nat.TARGET_LABELS
    with torch.cuda.device(logits.device):
        nat.check(nat.lib.ww_distill_loss_f32(_ptr(logits), _ptr(teacher_logits), None if targets is None else _ptr(targets), kind,
                                              logits.shape[0], None if opts is None else C.byref(opts), alpha, temperature,
                                              None if dlogits is None else _ptr(dlogits), None if loss is None else _ptr(loss),
                                              None if stats is None else _ptr(stats),
                                              None if distill_stats is None else _ptr(distill_stats), _stream()))


def distill_loss(logits: torch.Tensor, teacher_logits: torch.Tensor, targets=None, stats=None, distill_stats=None, grad: bool = True, *,
                 alpha=0.5, temperature=2.0, weight=None, label_smoothing=0.0, ignore_index=-100, reduction="mean", focal_gamma=None):
    """L = (1 - alpha) H(logits, targets) + alpha T^2 KD(logits, teacher_logits), Hinton's distillation loss, in one launch:
    (loss [] float32, dlogits [n, 2] or None with grad=False).  KD is F.kl_div(log_softmax(z / T), softmax(zt / T), "batchmean") over
    the rows whose teacher logits are both finite.  `targets`: int64 labels [n] or [n, 1] (H as in ce_loss with the keyword options,
    labels equal to ignore_index ignored), float32 class probabilities [n, 2] (H as in soft_ce_loss), or None -- unlabelled audio,
    L = T^2 KD and alpha is not read.  Under "mean" each term is divided by its own denominator; a term without a counted row adds
    exactly 0, and when neither has one the loss is NaN and the gradient all zeros.  `stats` as in ce_loss; `distill_stats`
    (ops.new_distill_stats) accumulates the two terms, the student-teacher agreement and the teacher's accuracy.  A bad option, alpha
    outside [0, 1] or a temperature that is not finite and > 0 raises ValueError before any device call."""
    from .loss import check_distillation
    check_distillation(alpha, temperature)
    if targets is not None and not isinstance(targets, torch.Tensor):
        raise TypeError(f"targets: expected a torch.Tensor or None, got {type(targets).__name__}")
    opts = distill_opts(targets, weight, label_smoothing, ignore_index, reduction, focal_gamma)
    _check_logits(logits)
    _check_teacher_logits(logits, teacher_logits)
    if targets is not None and targets.dtype == torch.float32:
        _check_soft(logits, targets)
    elif targets is not None:
        targets = _check_ce(logits, targets)
    if stats is not None:
        _check_stats(stats, logits)
    if distill_stats is not None:
        _check_distill_stats(distill_stats, logits)
    loss, dlogits = torch.empty((), device=logits.device, dtype=torch.float32), torch.empty_like(logits) if grad else None
    distill_loss_into(logits, teacher_logits, targets, dlogits, loss, stats, distill_stats, alpha=alpha, temperature=temperature,
                      opts=opts)                             # None: every option at its default, which the keywords' defaults repeat
    return loss, dlogits


def _check_mixup(mel, labels, partner, lam):
    if not isinstance(mel, torch.Tensor):
        raise TypeError(f"mel: expected a torch.Tensor, got {type(mel).__name__}")
    if mel.device.type != "cuda":
        raise RuntimeError(f"mel is on {mel.device}: this path has no CPU implementation; move it to the MI355X (`.cuda()`)")
    if mel.dtype != torch.float32 or not ((mel.dim() == 4 and mel.shape[1] == 1 and mel.shape[2] == N_MELS) or
                                          (mel.dim() == 3 and mel.shape[1] == N_MELS)) or not mel.is_contiguous() or mel.shape[0] == 0:
        raise ValueError(f"mel: expected contiguous float32 [B >= 1, 1, {N_MELS}, T] or [B, {N_MELS}, T], got {mel.dtype} {tuple(mel.shape)}")
    B = int(mel.shape[0])
    _check_frames(int(mel.shape[-1]), "mel")
    for name, t, dtype in (("labels", labels, torch.int64), ("partner", partner, torch.int32), ("lam", lam, torch.float32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != mel.device:
            raise TypeError(f"{name}: expected a {dtype} tensor on {mel.device}")
    if labels.dim() == 2 and labels.shape[1] == 1:
        labels = labels[:, 0]
    for name, t in (("labels", labels), ("partner", partner), ("lam", lam)):
        if t.dim() != 1 or t.shape[0] != B or (B > 1 and t.stride(0) != 1):
            raise ValueError(f"{name}: expected [{B}] with unit stride, got {tuple(t.shape)}")
    return labels


def _check_mixup_out(mel, out, targets):
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.shape != mel.shape or out.device != mel.device
            or not out.is_contiguous()):
        raise ValueError("out: expected a contiguous float32 tensor of mel's shape on mel's device")
    if (not isinstance(targets, torch.Tensor) or targets.dtype != torch.float32 or tuple(targets.shape) != (mel.shape[0], 2)
            or targets.device != mel.device or not targets.is_contiguous()):
        raise ValueError(f"targets: expected a contiguous float32 [{mel.shape[0]}, 2] tensor on mel's device")


def mixup_into(mel, labels, partner, lam, out, targets) -> None:
    """ww_mixup_f32 on caller-owned `out` (like mel, not overlapping it) and `targets` [B, 2]; arguments as ops.mixup takes them.
    Allocates nothing on the device."""
    labels = _check_mixup(mel, labels, partner, lam)
    _check_mixup_out(mel, out, targets)
    with torch.cuda.device(mel.device):
        nat.check(nat.lib.ww_mixup_f32(_ptr(mel), _ptr(out), mel.shape[0], int(mel.shape[-1]), _ptr(labels), _ptr(partner), _ptr(lam),
                                       _ptr(targets), _stream()))


def mixup(mel: torch.Tensor, labels: torch.Tensor, partner: torch.Tensor, lam: torch.Tensor, out=None):
    """mel float32 [B, 1, 80, T] or [B, 80, T] on the GPU, contiguous, T <= 63; labels int64 [B] or [B, 1], partner int32 [B] and lam
    float32 [B] on the same device -> (out like mel, targets float32 [B, 2]).  Row i with lam[i] == 1 is copied bit for bit; any other
    row becomes fmaf(lam, mel[i], (1 - lam) * mel[partner[i]]) and its target the same mix of the two one-hot labels.  A label outside
    {0, 1} on a row (or on the partner of a mixed row) and a partner outside [0, B) give a (NaN, NaN) target, which ops.soft_ce_loss counts
    as a bad label.  Out of place: `out` must not overlap mel."""
    labels = _check_mixup(mel, labels, partner, lam)
    if out is None:
        out = torch.empty_like(mel)
    targets = torch.empty((mel.shape[0], 2), device=mel.device, dtype=torch.float32)
    mixup_into(mel, labels, partner, lam, out, targets)
    return out, targets


# ---- loss-ranked selection: train on the hardest k of a batch (csrc/ww_select.hip) -------------------------
SELECT_STATS_FIELDS = ("batches", "candidates", "kept", "candidate_positive", "kept_positive", "unranked", "kept_unranked", "threshold_bits")
SELECT_MAX_ROWS = nat.SELECT_MAX_ROWS


def new_select_stats(device) -> torch.Tensor:
    """A zeroed ww_select_stats record in device memory: eight int64 words; `.zero_()` starts a new epoch."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"selection stats on {device}: this path has no CPU implementation")
    return torch.zeros(len(SELECT_STATS_FIELDS), device=device, dtype=torch.int64)


def read_select_stats(stats: torch.Tensor) -> dict:
    """The record on the host: the seven counters as int and `threshold`, the float64 the record's last word holds (the smallest
    selected score of the newest call; -inf when a rank-0 row was selected; NaN before the first call).  One device-to-host copy (none
    for a record that already is on the host)."""
    host = stats.cpu()
    out = {k: int(v) for k, v in zip(SELECT_STATS_FIELDS[:-1], host[:-1].tolist())}
    out["threshold"] = float(host[-1:].view(torch.float64).item()) if out["batches"] else float("nan")
    return out


def hard_select_workspace_bytes(n: int) -> int:
    return nat.check(nat.lib.ww_hard_select_workspace_bytes(int(n)))


def _keep_class(keep_class) -> int:
    if keep_class is None:
        return -1
    if isinstance(keep_class, bool) or not isinstance(keep_class, int) or keep_class not in (0, 1):
        raise ValueError(f"keep_class {keep_class!r}: expected None, 0 or 1")
    return keep_class


def hard_select_into(logits, targets, keep, sel, scores, stats, workspace, *, opts=None, keep_class=None) -> None:
    """ww_hard_select_f32 on caller-owned buffers: logits float32 [n, 2] contiguous, `targets` int64 labels [n] (unit stride) or float32
    probabilities [n, 2]; `sel` int64 [>= keep] receives the kept rows in rising index, `scores` float64 [>= n] (or None) every row's
    score, `stats` the record of ops.new_select_stats (or None); `workspace` uint8 of hard_select_workspace_bytes(n).  `opts`: the
    criterion's options as ops.loss_opts / ops.soft_loss_opts made them (None: the plain rule).  One launch, no wait, no allocation."""
    kind = nat.TARGET_PROBS if targets.dtype == torch.float32 else nat.TARGET_LABELS
    with torch.cuda.device(logits.device):
        nat.check(nat.lib.ww_hard_select_f32(_ptr(logits), _ptr(targets), kind, logits.shape[0], int(keep), None if opts is None else C.byref(opts),
                                             _keep_class(keep_class), _ptr(sel), None if scores is None else _ptr(scores),
                                             None if stats is None else _ptr(stats), _ptr(workspace), _stream()))


def select_rows_into(x, sel, x_out, targets=None, targets_out=None, entries=None, entries_out=None, labels=None, labels_out=None) -> None:
    """ww_select_rows_f32 on caller-owned buffers: row sel[j] of `x` (float32 [n, 1, 80, T] or [n, 80, T], T <= 32, contiguous), of
    `targets` (int64 [n] or float32 [n, 2]), of `entries` and of `labels` (int64 [n]) -> row j of the matching output, j < len(sel).
    Every pair but x's may be None.  One launch, no wait, no allocation; out of place."""
    if not (x.is_contiguous() and x_out.is_contiguous() and sel.is_contiguous()) or tuple(x_out.shape) != (sel.shape[0],) + tuple(x.shape[1:]):
        raise ValueError(f"select_rows_into: x, x_out and sel must be contiguous and x_out {(sel.shape[0],) + tuple(x.shape[1:])}, "
                         f"got {tuple(x_out.shape)}")
    kind = nat.TARGET_PROBS if targets is not None and targets.dtype == torch.float32 else nat.TARGET_LABELS
    opt = lambda t: None if t is None else _ptr(t)           # noqa: E731
    with torch.cuda.device(x.device):
        nat.check(nat.lib.ww_select_rows_f32(_ptr(x), x.shape[0], int(x.shape[-1]), _ptr(sel), sel.shape[0], _ptr(x_out), opt(targets), kind,
                                             opt(targets_out), opt(entries), opt(entries_out), opt(labels), opt(labels_out), _stream()))


def hard_select(logits: torch.Tensor, targets: torch.Tensor, keep: int, *, opts=None, keep_class=None):
    """The `keep` hardest rows of a batch: (sel int64 [keep] in rising row index, scores float64 [n]).  logits float32 [n, 2] and
    `targets` -- int64 labels [n] or [n, 1], or float32 class probabilities [n, 2] -- on the GPU, n <= 65536.  A row's score is the
    per-clip loss of the criterion `opts` describes (ops.loss_opts(...) for labels, ops.soft_loss_opts(...) for probabilities; None:
    plain cross-entropy), before the mean's division; rows are ranked by (rank class desc, score desc, index asc) with rank class 2 for
    counting rows of class `keep_class`, 1 for other counting rows with finite logits and score, 0 for the rest (score -inf).
    Allocates its outputs and a workspace; ops.hard_select_into is the form that allocates nothing."""
    _check_logits(logits)
    if isinstance(targets, torch.Tensor) and targets.dtype == torch.float32:
        _check_soft(logits, targets)
    else:
        targets = _check_ce(logits, targets)
    n = logits.shape[0]
    if isinstance(keep, bool) or not isinstance(keep, int) or not 1 <= keep <= n:
        raise ValueError(f"keep {keep!r}: expected an integer in 1..{n}")
    _keep_class(keep_class)
    if n > SELECT_MAX_ROWS:
        raise ValueError(f"hard_select: {n} rows; the selection kernel takes up to {SELECT_MAX_ROWS}")
    sel = torch.empty(keep, device=logits.device, dtype=torch.int64)
    scores = torch.empty(n, device=logits.device, dtype=torch.float64)
    ws = torch.empty(hard_select_workspace_bytes(n), device=logits.device, dtype=torch.uint8)
    hard_select_into(logits, targets, keep, sel, scores, None, ws, opts=opts, keep_class=keep_class)
    ws.record_stream(torch.cuda.current_stream())
    return sel, scores


# ---- clip evaluation as device counters (csrc/ww_metrics.hip) ---------------------------------------------
class ClipMetricsState:
    """A ww_clip_metrics record in device memory (`buffer`, int64 words) with the probability thresholds it was made for and their float32
    margins as the library computed them."""
    __slots__ = ("buffer", "thresholds", "margins")

    def __init__(self, buffer, thresholds, margins):
        self.buffer, self.thresholds, self.margins = buffer, thresholds, margins

    @property
    def device(self):
        return self.buffer.device


def new_clip_metrics(device, thresholds=(0.8,)) -> ClipMetricsState:
    """A zeroed evaluation record on `device` with up to 8 operating points, each a probability in (0, 1)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"clip metrics on {device}: this path has no CPU implementation")
    thresholds = tuple(float(p) for p in thresholds)
    if len(thresholds) > nat.METRICS_MAX_THRESHOLDS:
        raise ValueError(f"thresholds: at most {nat.METRICS_MAX_THRESHOLDS} operating points, got {len(thresholds)}")
    for p in thresholds:
        if not 0.0 < float(np.float32(p)) < 1.0:
            raise ValueError(f"thresholds: {p!r} is not a probability in (0, 1)")
    if len(set(np.float32(p) for p in thresholds)) != len(thresholds):
        raise ValueError(f"thresholds: {thresholds} repeats an operating point")
    nbytes = nat.check(nat.lib.ww_clip_metrics_bytes())
    assert nbytes == C.sizeof(nat.ClipMetrics) and nbytes % 8 == 0
    margins = np.array([nat.lib.ww_clip_metrics_margin_host(p) for p in thresholds], np.float32)
    host = (C.c_float * max(1, len(thresholds)))(*thresholds)
    with torch.cuda.device(device):
        buf = torch.empty(nbytes // 8, device=device, dtype=torch.int64)
        nat.check(nat.lib.ww_clip_metrics_init(_ptr(buf), host, len(thresholds), _stream()))
    return ClipMetricsState(buf, thresholds, margins)


def _check_metrics_state(state, like=None) -> None:
    if not isinstance(state, ClipMetricsState):
        raise TypeError(f"state: expected what ops.new_clip_metrics() makes, got {type(state).__name__}")
    if like is not None and state.device != like.device:
        raise RuntimeError(f"state on {state.device}, logits on {like.device}")


def clip_metrics_update_into(logits, labels, state) -> None:
    """ww_clip_metrics_update_f32 on checked arguments (`labels` as _check_ce returns them): one launch, nothing else."""
    with torch.cuda.device(logits.device):
        nat.check(nat.lib.ww_clip_metrics_update_f32(_ptr(logits), _ptr(labels), logits.shape[0], _ptr(state.buffer), _stream()))


def clip_metrics_update(logits: torch.Tensor, labels: torch.Tensor, state: ClipMetricsState) -> None:
    """Add a batch to the record: logits [n, 2] float32 and labels [n] or [n, 1] int64 on the GPU (the checks of `ce_loss`).  One launch
    in stream order; nothing waits for the device."""
    labels = _check_ce(logits, labels)
    _check_metrics_state(state, logits)
    clip_metrics_update_into(logits, labels, state)


def reset_clip_metrics(state: ClipMetricsState) -> None:
    """Zero the counters and keep the operating points."""
    _check_metrics_state(state)
    with torch.cuda.device(state.device):
        nat.check(nat.lib.ww_clip_metrics_reset(_ptr(state.buffer), _stream()))


def read_clip_metrics(state: ClipMetricsState):
    """The record on the host as a metrics.ClipReport.  The one device-to-host copy of an evaluation."""
    from .metrics import ClipReport
    _check_metrics_state(state)
    host = state.buffer.cpu().numpy()
    rec = nat.ClipMetrics.from_buffer_copy(host.tobytes())
    k = int(rec.n_thresholds)
    margins = np.ctypeslib.as_array(rec.margin).copy()[:k]
    if k != len(state.thresholds) or not np.array_equal(margins, state.margins):
        raise RuntimeError("the record's operating points are not the ones it was made with: was the buffer overwritten?")
    report = ClipReport.from_counts(np.ctypeslib.as_array(rec.argmax).copy(), hist=np.ctypeslib.as_array(rec.hist).copy(), margins=margins,
                                    at=np.ctypeslib.as_array(rec.at).copy()[:k], bad_labels=int(rec.bad_labels),
                                    nonfinite=int(rec.nonfinite), thresholds=state.thresholds)
    report.clips_seen, report.batches = int(rec.total), int(rec.batches)
    return report


# ---- clip ledger: a per-clip training record as device integers (csrc/ww_ledger.hip) ----------------------
class ClipLedgerState:
    """A clip ledger in device memory: `buffer` (int64 words: a ww_ledger_header, then `n_entries` ww_ledger_entry records)."""
    __slots__ = ("buffer", "n_entries")

    def __init__(self, buffer, n_entries):
        self.buffer, self.n_entries = buffer, n_entries

    @property
    def device(self):
        return self.buffer.device


def new_clip_ledger(device, n_entries) -> ClipLedgerState:
    """A cleared ledger of `n_entries` records (0..2^28) on `device`."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"clip ledger on {device}: this path has no CPU implementation")
    if isinstance(n_entries, bool) or int(n_entries) != n_entries or not 0 <= int(n_entries) <= nat.LEDGER_MAX_ENTRIES:
        raise ValueError(f"n_entries {n_entries!r}: expected an integer in 0..2^28")
    n_entries = int(n_entries)
    nbytes = nat.check(nat.lib.ww_clip_ledger_bytes(n_entries))
    assert nbytes == C.sizeof(nat.LedgerHeader) + n_entries * C.sizeof(nat.LedgerEntry) and nbytes % 8 == 0
    with torch.cuda.device(device):
        state = ClipLedgerState(torch.empty(nbytes // 8, device=device, dtype=torch.int64), n_entries)
    clip_ledger_reset(state)
    return state


def _check_ledger_state(state, like=None) -> None:
    if not isinstance(state, ClipLedgerState):
        raise TypeError(f"state: expected what ops.new_clip_ledger() makes, got {type(state).__name__}")
    if like is not None and state.device != like.device:
        raise RuntimeError(f"ledger on {state.device}, logits on {like.device}")


def clip_ledger_reset(state: ClipLedgerState) -> None:
    """ww_clip_ledger_init: the header written and every record cleared, whatever the buffer held."""
    _check_ledger_state(state)
    with torch.cuda.device(state.device):
        nat.check(nat.lib.ww_clip_ledger_init(_ptr(state.buffer), state.n_entries, _stream()))


def clip_ledger_update_into(logits, labels, entries, state, epoch=-1) -> None:
    """ww_clip_ledger_update_f32 on checked arguments (`labels` as _check_ce returns them, `entries` int64 [n] on the device, unit
    stride): one launch, nothing else."""
    with torch.cuda.device(logits.device):
        nat.check(nat.lib.ww_clip_ledger_update_f32(_ptr(logits), _ptr(labels), _ptr(entries), logits.shape[0], int(epoch),
                                                    _ptr(state.buffer), state.n_entries, _stream()))


def clip_ledger_update(logits: torch.Tensor, labels: torch.Tensor, entries: torch.Tensor, state: ClipLedgerState, epoch: int = -1) -> None:
    """Add a batch to the ledger: logits [n, 2] float32, labels [n] or [n, 1] int64 (the checks of `ce_loss`) and entries [n] int64, all
    on the GPU; `epoch` in 0..63, or -1 for no epoch bit.  A negative entry is skipped, one >= n_entries is counted in `bad_entries`
    and written nowhere.  One launch in stream order; nothing waits for the device."""
    labels = _check_ce(logits, labels)
    _check_ledger_state(state, logits)
    if not isinstance(entries, torch.Tensor) or entries.dtype != torch.int64:
        raise TypeError("entries: expected an int64 torch.Tensor")
    if entries.device != logits.device:
        raise RuntimeError(f"entries on {entries.device}, logits on {logits.device}")
    if entries.dim() != 1 or entries.shape[0] != logits.shape[0]:
        raise ValueError(f"entries: expected [{logits.shape[0]}], got {tuple(entries.shape)}")
    if isinstance(epoch, bool) or int(epoch) != epoch or not -1 <= int(epoch) < nat.LEDGER_MAX_EPOCHS:
        raise ValueError(f"epoch {epoch!r}: expected 0..63, or -1 for no epoch bit")
    if entries.stride(0) != 1 and entries.shape[0] != 1:
        entries = entries.contiguous()
    clip_ledger_update_into(logits, labels, entries, state, epoch)


def read_clip_ledger(state: ClipLedgerState):
    """The ledger on the host as a ledger.LedgerReport.  One device-to-host copy."""
    from .ledger import LedgerReport
    _check_ledger_state(state)
    return LedgerReport.from_buffer(state.buffer.cpu().numpy(), state.n_entries)


def adam_table(params, grads, exp_avgs, exp_avg_sqs):
    """Four equally long lists of float32 GPU tensors -> a ctypes array of _native.AdamTensor (at most 16 entries).  A grads-only table
    (the other three None) is what grad_norm reads."""
    n = len(grads)
    if not 1 <= n <= nat.ADAM_MAX_TENSORS:
        raise ValueError(f"{n} tensors: one launch takes 1..{nat.ADAM_MAX_TENSORS}")
    cols = [grads if c is None else c for c in (params, grads, exp_avgs, exp_avg_sqs)]
    if any(len(c) != n for c in cols):
        raise ValueError("params, grads, exp_avgs and exp_avg_sqs differ in length")
    tab = (nat.AdamTensor * n)()
    for k, (p, g, m, v) in enumerate(zip(*cols)):
        for name, t in (("param", p), ("grad", g), ("exp_avg", m), ("exp_avg_sq", v)):
            _require_cuda_f32(t, f"{name} {k}")
            if not t.is_contiguous():
                raise RuntimeError(f"{name} {k} is not contiguous")
            if t.numel() != p.numel() or t.device != p.device:
                raise ValueError(f"{name} {k}: {t.numel()} elements on {t.device}, its parameter has {p.numel()} on {p.device}")
        if p.numel() == 0:
            raise ValueError(f"param {k} is empty")
        tab[k].p, tab[k].g, tab[k].m, tab[k].v, tab[k].n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
    return tab


def adam_launch(table, device, lr, betas, eps, weight_decay, step, grad_scale=None) -> None:
    """ww_adam_step_f32 on a prepared adam_table (FusedAdam and the trainer keep theirs between steps).  Allocates nothing."""
    with torch.cuda.device(device):
        nat.check(nat.lib.ww_adam_step_f32(table, len(table), float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                           int(step), None if grad_scale is None else _ptr(grad_scale), _stream()))


def adam_step(params, grads, exp_avgs, exp_avg_sqs, *, lr, betas, eps, weight_decay, step, grad_scale=None) -> None:
    """One launch of torch's single-tensor Adam over up to 16 tensors, in place (ww_adam_step_f32).  `step` is the 1-based count of this
    update; `grad_scale` (float32 [1] on the GPU, grad_norm's scale) multiplies every gradient inside the kernel.  The parameters are
    written behind autograd's back: their version counters do not move (optim.FusedAdam bumps them)."""
    tab = adam_table(params, grads, exp_avgs, exp_avg_sqs)
    if grad_scale is not None:
        _require_cuda_f32(grad_scale, "grad_scale")
        if grad_scale.numel() != 1 or grad_scale.device != grads[0].device:
            raise ValueError("grad_scale: expected one float32 on the gradients' device")
    adam_launch(tab, grads[0].device, lr, betas, eps, weight_decay, step, grad_scale)


def average_pointers(avgs, params=None):
    """A list of float32 GPU tensors (the averaged copies of up to 16 parameters) -> the ctypes pointer array ww_adam_avg_step_f32 and
    ww_weight_average_f32 take beside an adam_table.  With `params`, every average must have its parameter's size and device."""
    n = len(avgs)
    if not 1 <= n <= nat.ADAM_MAX_TENSORS:
        raise ValueError(f"{n} tensors: one launch takes 1..{nat.ADAM_MAX_TENSORS}")
    if params is not None and len(params) != n:
        raise ValueError("params and avgs differ in length")
    ptrs = (C.c_void_p * n)()
    for k, a in enumerate(avgs):
        _require_cuda_f32(a, f"average {k}")
        if not a.is_contiguous():
            raise RuntimeError(f"average {k} is not contiguous")
        if params is not None and (a.numel() != params[k].numel() or a.device != params[k].device):
            raise ValueError(f"average {k}: {a.numel()} elements on {a.device}, its parameter has {params[k].numel()} on {params[k].device}")
        ptrs[k] = a.data_ptr()
    return ptrs


def adam_average_launch(table, avg_ptrs, device, lr, betas, eps, weight_decay, step, avg_weight, grad_scale=None) -> None:
    """ww_adam_avg_step_f32 on a prepared adam_table and its average_pointers: the Adam step and the averaging of its result in one
    launch.  `avg_weight` comes from average.update_weight.  Allocates nothing."""
    if len(avg_ptrs) != len(table):
        raise ValueError(f"{len(avg_ptrs)} averages for a table of {len(table)}")
    with torch.cuda.device(device):
        nat.check(nat.lib.ww_adam_avg_step_f32(table, avg_ptrs, len(table), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                               float(weight_decay), int(step), None if grad_scale is None else _ptr(grad_scale),
                                               float(avg_weight), _stream()))


def adam_average_step(params, grads, exp_avgs, exp_avg_sqs, avgs, *, lr, betas, eps, weight_decay, step, avg_weight, grad_scale=None) -> None:
    """adam_step with the averaging of its result in the same launch (ww_adam_avg_step_f32): avgs[k] <- lerp(avgs[k], params[k], avg_weight)
    with the parameter as this step leaves it.  Version counters do not move (optim.FusedAdam bumps them)."""
    tab = adam_table(params, grads, exp_avgs, exp_avg_sqs)
    ptrs = average_pointers(avgs, params)
    if grad_scale is not None:
        _require_cuda_f32(grad_scale, "grad_scale")
        if grad_scale.numel() != 1 or grad_scale.device != grads[0].device:
            raise ValueError("grad_scale: expected one float32 on the gradients' device")
    adam_average_launch(tab, ptrs, grads[0].device, lr, betas, eps, weight_decay, step, avg_weight, grad_scale)


def weight_average_launch(table, avg_ptrs, device, avg_weight) -> None:
    """ww_weight_average_f32 on a prepared table (only its p and n are read) and its average_pointers.  Allocates nothing."""
    if len(avg_ptrs) != len(table):
        raise ValueError(f"{len(avg_ptrs)} averages for a table of {len(table)}")
    with torch.cuda.device(device):
        nat.check(nat.lib.ww_weight_average_f32(table, avg_ptrs, len(table), float(avg_weight), _stream()))


def weight_average(params, avgs, weight: float) -> None:
    """avgs[k] <- lerp(avgs[k], params[k], weight) in place, one launch per 16 tensors (ww_weight_average_f32): weight 1 copies without
    reading the average, weight 0 leaves it alone.  The averages are written behind autograd's back: their version counters do not
    move (average.WeightAverage bumps them)."""
    params, avgs = list(params), list(avgs)
    if len(params) != len(avgs):
        raise ValueError("params and avgs differ in length")
    for i in range(0, len(params), nat.ADAM_MAX_TENSORS):
        ps = params[i:i + nat.ADAM_MAX_TENSORS]
        weight_average_launch(adam_table(ps, ps, ps, ps), average_pointers(avgs[i:i + nat.ADAM_MAX_TENSORS], ps), ps[0].device, weight)


def grad_norm_workspace(table, device) -> torch.Tensor:
    return torch.empty(max(256, nat.check(nat.lib.ww_grad_norm_workspace_bytes(table, len(table)))), device=device, dtype=torch.uint8)


def grad_norm_launch(table, device, max_norm, norm, scale, workspace) -> None:
    """ww_grad_norm_f32 on a prepared table and caller-owned outputs.  Allocates nothing."""
    with torch.cuda.device(device):
        nat.check(nat.lib.ww_grad_norm_f32(table, len(table), float(max_norm), _ptr(norm), _ptr(scale), _ptr(workspace), _stream()))


def grad_norm(grads, max_norm: float):
    """(norm float64 [1], scale float32 [1]) on the GPU: the global L2 norm over `grads` (up to 16 float32 tensors) and clip_grad_norm_'s
    coefficient min(1, max_norm / (norm + 1e-6)); adam_step(grad_scale=scale) applies it without a host wait."""
    tab = adam_table(None, grads, None, None)
    device = grads[0].device
    norm = torch.empty(1, device=device, dtype=torch.float64)
    scale = torch.empty(1, device=device, dtype=torch.float32)
    grad_norm_launch(tab, device, max_norm, norm, scale, grad_norm_workspace(tab, device))
    return norm, scale


# ---- post-training weight quantisation (csrc/ww_quant.hip) -------------------------------------------------
def check_quant_bits(bits) -> int:
    if isinstance(bits, bool) or not isinstance(bits, int) or not 2 <= bits <= 8:
        raise ValueError(f"bits {bits!r}: expected an integer in 2..8")
    return bits


def quant_groups(t: torch.Tensor, per_channel: bool = True):
    """(rows, cols) of a weight tensor as ww_quant_weights_f32 groups it: one group per slice of the first dimension (an output channel, a
    gate row, a row of fc.weight), or the whole tensor as one group in per-tensor mode and for anything with fewer than two dimensions."""
    if per_channel and t.dim() >= 2:
        return int(t.shape[0]), t.numel() // max(1, int(t.shape[0]))
    return 1, t.numel()


def _quant_mode_list(per_channel, n):
    modes = [bool(per_channel)] * n if isinstance(per_channel, (bool, int)) else [bool(m) for m in per_channel]
    if len(modes) != n:
        raise ValueError(f"per_channel: {len(modes)} entries for {n} tensors")
    return modes


def _quant_entry(k, w, per_channel, outputs):
    """Check weight `k` and its outputs [(name, tensor or None, dtype, elements per row or None for the weight's size)] -> (rows, cols)."""
    _require_cuda_f32(w, f"weight {k}")
    if not w.is_contiguous():
        raise RuntimeError(f"weight {k} is not contiguous")
    if w.numel() == 0:
        raise ValueError(f"weight {k} is empty")
    rows, cols = quant_groups(w, per_channel)
    for name, t, dtype, per_row in outputs:
        if t is None:
            continue
        numel = w.numel() if per_row is None else per_row * rows
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise TypeError(f"{name} {k}: expected a {dtype} torch.Tensor")
        if t.device != w.device:
            raise RuntimeError(f"{name} {k} on {t.device}, its weight on {w.device}")
        if t.numel() != numel or not t.is_contiguous():
            raise ValueError(f"{name} {k}: expected {numel} contiguous elements, got {tuple(t.shape)}")
    return rows, cols


def _quant_columns(weights, columns, what):
    weights = list(weights)
    n = len(weights)
    if not 1 <= n <= nat.QUANT_MAX_TENSORS:
        raise ValueError(f"{n} tensors: one launch takes 1..{nat.QUANT_MAX_TENSORS}")
    cols_of = [[None] * n if c is None else list(c) for c in columns]
    if any(len(c) != n for c in cols_of):
        raise ValueError(f"{what} differ in length")
    return weights, n, cols_of


def quant_table(weights, scales, qs=None, deqs=None, errs=None, bads=None, per_channel=True):
    """Up to 16 float32 GPU weight tensors and their outputs -> a ctypes array of _native.QuantTensor.  Per tensor of rows x cols
    (quant_groups; `per_channel` a bool or one per tensor): scale float32 [rows]; q int8, deq float32 of the weight's size; err float64
    [rows, 3]; bad int32 [rows].  Each of qs, deqs, errs, bads may be None, and so may single entries of them."""
    weights, n, cols_of = _quant_columns(weights, (scales, qs, deqs, errs, bads), "weights, scales, qs, deqs, errs and bads")
    modes = _quant_mode_list(per_channel, n)
    tab = (nat.QuantTensor * n)()
    for k, w in enumerate(weights):
        scale, q, deq, err, bad = (c[k] for c in cols_of)
        rows, cols = _quant_entry(k, w, modes[k], (("scale", scale, torch.float32, 1), ("q", q, torch.int8, None), ("deq", deq, torch.float32, None),
                                                   ("err", err, torch.float64, 3), ("bad", bad, torch.int32, 1)))
        if scale is None:
            raise TypeError(f"scale {k}: expected a float32 tensor [{rows}]")
        e = tab[k]
        e.w, e.scale, e.rows, e.cols = w.data_ptr(), scale.data_ptr(), rows, cols
        e.q, e.deq, e.err, e.bad = (None if t is None else t.data_ptr() for t in (q, deq, err, bad))
    return tab


def quantize_weights_launch(table, device, bits) -> None:
    """ww_quant_weights_f32 on a prepared quant_table (quant.WeightQuant keeps its tables between updates).  Allocates nothing."""
    with torch.cuda.device(device):
        nat.check(nat.lib.ww_quant_weights_f32(table, len(table), int(bits), _stream()))


def quantize_weights_into(weights, scales, qs=None, deqs=None, errs=None, bads=None, *, bits=8, per_channel=True) -> None:
    """Quantise `weights` into caller-owned outputs (quant_table has the shapes), one launch per 16 tensors, in stream order; nothing
    waits for the device.  The outputs are written behind autograd's back: version counters do not move (quant.WeightQuant bumps them)."""
    bits = check_quant_bits(bits)
    weights = list(weights)
    modes = _quant_mode_list(per_channel, len(weights))
    outs = [[None] * len(weights) if c is None else list(c) for c in (scales, qs, deqs, errs, bads)]
    if any(len(c) != len(weights) for c in outs):
        raise ValueError("weights, scales, qs, deqs, errs and bads differ in length")
    step = nat.QUANT_MAX_TENSORS
    tables = [quant_table(weights[i:i + step], *(c[i:i + step] for c in outs), per_channel=modes[i:i + step]) for i in range(0, len(weights), step)]
    for i, tab in enumerate(tables):                         # every table was checked before the first launch
        quantize_weights_launch(tab, weights[i * step].device, bits)


def quantize_weights(tensors, bits=8, per_channel=True):
    """[(q int8, scale float32 [rows], deq float32, err float64 [rows, 3], bad int32 [rows])] for a list of float32 GPU weight tensors:
    symmetric `bits`-bit quantisation per output channel / row (per_channel=True) or per tensor, by the rule of include/wakeword_amd.h
    (ww_quant_weights_f32).  q and deq have the weight's shape; err rows are (sum w^2, sum (w - deq)^2, max |w - deq|)."""
    bits = check_quant_bits(bits)
    tensors = list(tensors)
    modes = _quant_mode_list(per_channel, len(tensors))
    for k, w in enumerate(tensors):
        _require_cuda_f32(w, f"weight {k}")
    out = []
    for w, m in zip(tensors, modes):
        rows, _ = quant_groups(w, m)
        out.append((torch.empty(w.shape, device=w.device, dtype=torch.int8), torch.empty(rows, device=w.device, dtype=torch.float32),
                    torch.empty(w.shape, device=w.device, dtype=torch.float32), torch.empty((rows, 3), device=w.device, dtype=torch.float64),
                    torch.empty(rows, device=w.device, dtype=torch.int32)))
    if tensors:
        quantize_weights_into(tensors, *([o[j] for o in out] for j in (1, 0, 2, 3, 4)), bits=bits, per_channel=modes)
    return out


# ---- clipped scales and the straight-through estimator (csrc/ww_quant.hip) ---------------------------------
QUANT_CLIPS = ("max", "mse")


def check_quant_clip(clip) -> str:
    if clip not in QUANT_CLIPS:
        raise ValueError(f"clip {clip!r}: expected one of {QUANT_CLIPS}")
    return clip


def quant_clip_table(weights, scales, clips, qs=None, deqs=None, errs=None, bads=None, sats=None, cand_errs=None, per_channel=True):
    """quant_table for ww_quant_weights_clip_f32 and ww_quant_clip_search_f32 -> a ctypes array of _native.QuantClipTensor: per tensor
    also clip uint8 [rows] (read by the first, written by the second), sat int32 [rows] and cand_err float64 [rows, 48], both optional."""
    columns = (scales, clips, qs, deqs, errs, bads, sats, cand_errs)
    weights, n, cols_of = _quant_columns(weights, columns, "weights, scales, clips, qs, deqs, errs, bads, sats and cand_errs")
    modes = _quant_mode_list(per_channel, n)
    tab = (nat.QuantClipTensor * n)()
    for k, w in enumerate(weights):
        scale, clip, q, deq, err, bad, sat, cand = (c[k] for c in cols_of)
        rows, cols = _quant_entry(k, w, modes[k], (("scale", scale, torch.float32, 1), ("clip", clip, torch.uint8, 1), ("q", q, torch.int8, None),
                                                   ("deq", deq, torch.float32, None), ("err", err, torch.float64, 3), ("bad", bad, torch.int32, 1),
                                                   ("sat", sat, torch.int32, 1), ("cand_err", cand, torch.float64, nat.QUANT_CLIP_STEPS)))
        if scale is None or clip is None:
            raise TypeError(f"scale / clip {k}: expected a float32 and a uint8 tensor [{rows}]")
        e = tab[k]
        e.w, e.scale, e.clip, e.rows, e.cols = w.data_ptr(), scale.data_ptr(), clip.data_ptr(), rows, cols
        e.q, e.deq, e.err, e.bad, e.sat, e.cand_err = (None if t is None else t.data_ptr() for t in (q, deq, err, bad, sat, cand))
    return tab


def quantize_weights_clip_launch(table, device, bits) -> None:
    """ww_quant_weights_clip_f32 on a prepared quant_clip_table.  Allocates nothing."""
    with torch.cuda.device(device):
        nat.check(nat.lib.ww_quant_weights_clip_f32(table, len(table), int(bits), _stream()))


def quant_clip_search_launch(table, device, bits) -> None:
    """ww_quant_clip_search_f32 on a prepared quant_clip_table: writes clip, scale and, where given, cand_err.  Allocates nothing."""
    with torch.cuda.device(device):
        nat.check(nat.lib.ww_quant_clip_search_f32(table, len(table), int(bits), _stream()))


def quant_ste_table(weights, scales, grads, per_channel=True):
    """Up to 16 float32 GPU weight tensors, their stored scales float32 [rows] and their gradients (float32, the weight's size, modified in
    place) -> a ctypes array of _native.QuantSteTensor."""
    weights, n, (scales, grads) = _quant_columns(weights, (scales, grads), "weights, scales and grads")
    modes = _quant_mode_list(per_channel, n)
    tab = (nat.QuantSteTensor * n)()
    for k, w in enumerate(weights):
        rows, cols = _quant_entry(k, w, modes[k], (("scale", scales[k], torch.float32, 1), ("grad", grads[k], torch.float32, None)))
        if scales[k] is None or grads[k] is None:
            raise TypeError(f"scale / grad {k}: expected float32 tensors")
        e = tab[k]
        e.w, e.scale, e.g, e.rows, e.cols = w.data_ptr(), scales[k].data_ptr(), grads[k].data_ptr(), rows, cols
    return tab


def quant_ste_launch(table, device, bits) -> None:
    """ww_quant_ste_f32 on a prepared quant_ste_table.  Allocates nothing."""
    with torch.cuda.device(device):
        nat.check(nat.lib.ww_quant_ste_f32(table, len(table), int(bits), _stream()))


def _quant_chunks(n):
    return [slice(i, i + nat.QUANT_MAX_TENSORS) for i in range(0, n, nat.QUANT_MAX_TENSORS)]


def _quant_inputs(tensors, bits, per_channel):
    bits = check_quant_bits(bits)
    tensors = list(tensors)
    modes = _quant_mode_list(per_channel, len(tensors))
    for k, w in enumerate(tensors):
        _require_cuda_f32(w, f"weight {k}")
    return tensors, bits, modes


def quantize_weights_clip(tensors, clips, bits=8, per_channel=True):
    """[(q, scale, deq, err, bad, sat)] for float32 GPU weight tensors under the clipped rule of include/wakeword_amd.h
    (ww_quant_weights_clip_f32): `clips` holds one uint8 [rows] GPU tensor of candidate indices per weight; sat int32 [rows] counts the
    elements the clamp moved.  All-zero indices give quantize_weights' bits."""
    tensors, bits, modes = _quant_inputs(tensors, bits, per_channel)
    clips = list(clips)
    if len(clips) != len(tensors):
        raise ValueError("tensors and clips differ in length")
    out = []
    for w, m in zip(tensors, modes):
        rows, _ = quant_groups(w, m)
        new = lambda shape, dtype: torch.empty(shape, device=w.device, dtype=dtype)     # noqa: E731
        out.append((new(w.shape, torch.int8), new(rows, torch.float32), new(w.shape, torch.float32), new((rows, 3), torch.float64),
                    new(rows, torch.int32), new(rows, torch.int32)))
    tables = [quant_clip_table(tensors[c], [o[1] for o in out[c]], clips[c], [o[0] for o in out[c]], [o[2] for o in out[c]], [o[3] for o in out[c]],
                               [o[4] for o in out[c]], [o[5] for o in out[c]], per_channel=modes[c]) for c in _quant_chunks(len(tensors))]
    for c, tab in zip(_quant_chunks(len(tensors)), tables):      # every table was checked before the first launch
        quantize_weights_clip_launch(tab, tensors[c.start].device, bits)
    return out


def quant_clip_search(tensors, bits=8, per_channel=True, cand_err=True):
    """[(clip uint8 [rows], scale float32 [rows], cand_err float64 [rows, 48] or None)] for float32 GPU weight tensors
    (ww_quant_clip_search_f32): per row the squared error of every clip candidate, the first candidate with the smallest one and its scale."""
    tensors, bits, modes = _quant_inputs(tensors, bits, per_channel)
    out = []
    for w, m in zip(tensors, modes):
        rows, _ = quant_groups(w, m)
        out.append((torch.empty(rows, device=w.device, dtype=torch.uint8), torch.empty(rows, device=w.device, dtype=torch.float32),
                    torch.empty((rows, nat.QUANT_CLIP_STEPS), device=w.device, dtype=torch.float64) if cand_err else None))
    tables = [quant_clip_table(tensors[c], [o[1] for o in out[c]], [o[0] for o in out[c]], cand_errs=[o[2] for o in out[c]], per_channel=modes[c])
              for c in _quant_chunks(len(tensors))]
    for c, tab in zip(_quant_chunks(len(tensors)), tables):
        quant_clip_search_launch(tab, tensors[c.start].device, bits)
    return out


def quant_ste_(weights, scales, grads, bits=8, per_channel=True) -> None:
    """The straight-through estimator with clipping, in place on `grads` (ww_quant_ste_f32): where a finite weight lies outside its row's
    clipped range, |rint(w / scale)| > qmax, the gradient becomes +0.0; every other gradient keeps its bits.  Nothing waits."""
    weights, bits, modes = _quant_inputs(weights, bits, per_channel)
    scales, grads = list(scales), list(grads)
    if len(scales) != len(weights) or len(grads) != len(weights):
        raise ValueError("weights, scales and grads differ in length")
    tables = [quant_ste_table(weights[c], scales[c], grads[c], per_channel=modes[c]) for c in _quant_chunks(len(weights))]
    for c, tab in zip(_quant_chunks(len(weights)), tables):
        quant_ste_launch(tab, weights[c.start].device, bits)


# ---- SpecAugment: time and frequency masks on log-mel batches (csrc/ww_specaug.hip) ----------------------
def _spec_args(config, T: int):
    """(prob, n_freq, freq_max, n_time, time_max, fill_mode, fill_value) as ww_spec_augment_f32 takes them, for images of T frames."""
    check_spec_augment_config(config)
    fill = config.FILL
    if isinstance(fill, str):
        mode, value = {"mean": nat.SPEC_FILL_MEAN, "min": nat.SPEC_FILL_MIN}[fill], 0.0
    else:
        mode, value = nat.SPEC_FILL_VALUE, float(fill)
    return (float(config.PROB), int(config.FREQ_MASKS), int(config.FREQ_MASK_MAX), int(config.TIME_MASKS),
            int(float(config.TIME_MASK_MAX_FRACTION) * T), mode, value)


def _check_frames(T: int, what: str) -> None:
    if not 1 <= int(T) <= MAX_FRAMES:
        raise NotImplementedError(f"{what}: T = {T} frames; the masking kernel takes 1..{MAX_FRAMES} (2 s clips give 63)")


def spec_augment_records(seed: int, B: int, T: int, config=SpecAugmentConfig, device=None) -> torch.Tensor:
    """The records `spec_augment(mel, seed=seed, config=config)` applies to a batch of B images of T frames: int16 [B, 16] on the device,
    [f_start, f_width] x 4 then [t_start, t_width] x 4 per clip (ww_spec_augment_draw).  Clip c's record does not depend on B."""
    _check_frames(T, "spec_augment_records")
    if B < 0:
        raise ValueError(f"spec_augment_records: B = {B}")
    prob, n_freq, freq_max, n_time, time_max, _, _ = _spec_args(config, int(T))
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"spec_augment_records on {device}: this path has no CPU implementation")
    records = torch.empty((B, nat.SPEC_RECORD_INT16), device=device, dtype=torch.int16)
    with torch.cuda.device(device):
        nat.check(nat.lib.ww_spec_augment_draw(int(seed) & (2 ** 64 - 1), B, int(T), prob, n_freq, freq_max, n_time, time_max, _ptr(records),
                                               _stream()))
    return records


def pack_spec_plans(plans, T: int) -> np.ndarray:
    """A list of {"freq": [(start, width), ...], "time": [(start, width), ...]} (either key may be missing), one per clip ->
    numpy int16 [B, 16] in the kernel's record layout.  ValueError for more than 4 masks per axis, a negative start or width, or a
    mask that ends past the 80 mel bins or the T frames."""
    out = np.zeros((len(plans), nat.SPEC_RECORD_INT16), dtype=np.int16)
    for i, plan in enumerate(plans):
        for key, base, size in (("freq", 0, N_MELS), ("time", 2 * SPEC_MAX_MASKS, int(T))):
            masks = list(plan.get(key, ()))
            if len(masks) > SPEC_MAX_MASKS:
                raise ValueError(f"plan {i}: {len(masks)} {key} masks; a record holds {SPEC_MAX_MASKS}")
            for k, (start, width) in enumerate(masks):
                if int(start) != start or int(width) != width or start < 0 or width < 0 or start + width > size:
                    raise ValueError(f"plan {i}: {key} mask ({start}, {width}) does not lie inside 0..{size}")
                out[i, base + 2 * k], out[i, base + 2 * k + 1] = int(start), int(width)
    return out


def spec_augment(mel: torch.Tensor, records=None, *, seed=None, config=SpecAugmentConfig, out=None) -> torch.Tensor:
    """mel float32 [B, 1, 80, T] or [B, 80, T] on the GPU, contiguous, T <= 63 -> the same shape with blocks of mel bins and of frames
    replaced by the clip's mean, its minimum or a constant (config.FILL).  Exactly one of `records` (int16 [B, 16] on the device:
    spec_augment_records, or pack_spec_plans uploaded) and `seed` (the records are drawn inside the kernel from `config`) is given.
    `out=mel` masks in place; any other `out` is a contiguous tensor like mel that does not overlap it."""
    if not isinstance(mel, torch.Tensor):
        raise TypeError(f"mel: expected a torch.Tensor, got {type(mel).__name__}")
    if mel.device.type != "cuda":
        raise RuntimeError(f"mel is on {mel.device}: this path has no CPU implementation; move it to the MI355X (`.cuda()`)")
    if mel.dtype != torch.float32 or not ((mel.dim() == 4 and mel.shape[1] == 1 and mel.shape[2] == N_MELS) or
                                          (mel.dim() == 3 and mel.shape[1] == N_MELS)) or not mel.is_contiguous():
        raise ValueError(f"mel: expected contiguous float32 [B, 1, {N_MELS}, T] or [B, {N_MELS}, T], got {mel.dtype} {tuple(mel.shape)}")
    B, T = int(mel.shape[0]), int(mel.shape[-1])
    _check_frames(T, "mel")
    if (records is None) == (seed is None):
        raise ValueError("spec_augment: give exactly one of `records` and `seed`")
    prob, n_freq, freq_max, n_time, time_max, mode, value = _spec_args(config, T)
    if records is not None:
        if (not isinstance(records, torch.Tensor) or records.dtype != torch.int16 or tuple(records.shape) != (B, nat.SPEC_RECORD_INT16)
                or records.device != mel.device):
            raise ValueError(f"records: expected int16 [{B}, {nat.SPEC_RECORD_INT16}] on {mel.device}")
        records = records.contiguous()
        if records.data_ptr() % 16:
            records = records.clone()
        prob, n_freq, freq_max, n_time, time_max, seed = 0.0, 0, 0, 0, 0, 0
    if out is None:
        out = torch.empty_like(mel)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.shape != mel.shape or out.device != mel.device
          or not out.is_contiguous()):
        raise ValueError("out: expected a contiguous float32 tensor of mel's shape on mel's device")
    with torch.cuda.device(mel.device):
        nat.check(nat.lib.ww_spec_augment_f32(_ptr(mel), _ptr(out), B, T, None if records is None else _ptr(records), int(seed) & (2 ** 64 - 1),
                                              prob, n_freq, freq_max, n_time, time_max, mode, value, _stream()))
    return out


# ---- microphone-channel augmentation: random EQ, band limit, clipping (csrc/ww_channel.hip) -------------
CHANNEL_MIN_SAMPLES, CHANNEL_MAX_SAMPLES = 4000, 16383


def _channel_struct(config) -> "nat.ChannelConfig":
    """config.ChannelConfig (or a class with its fields; validated) as the struct ww_channel_draw / ww_channel_f32 take."""
    check_channel_config(config)
    g = nat.ChannelConfig()
    g.prob = config.PROB
    g.highpass_prob, (g.highpass_lo, g.highpass_hi) = config.HIGHPASS_PROB, config.HIGHPASS_HZ
    g.low_shelf_prob, (g.low_shelf_lo, g.low_shelf_hi) = config.LOW_SHELF_PROB, config.LOW_SHELF_HZ
    g.high_shelf_prob, (g.high_shelf_lo, g.high_shelf_hi) = config.HIGH_SHELF_PROB, config.HIGH_SHELF_HZ
    g.shelf_db = config.SHELF_DB
    g.peak_prob, (g.peak_lo, g.peak_hi), g.peak_db, (g.peak_q_lo, g.peak_q_hi) = config.PEAK_PROB, config.PEAK_HZ, config.PEAK_DB, config.PEAK_Q
    g.lowpass_prob, (g.lowpass_lo, g.lowpass_hi) = config.LOWPASS_PROB, config.LOWPASS_HZ
    g.drive_prob, (g.drive_lo, g.drive_hi) = config.DRIVE_PROB, config.DRIVE
    g.peaks = int(config.PEAKS)
    return g


def channel_records(seed: int, B: int, config=ChannelConfig, device=None) -> torch.Tensor:
    """The records `channel_effects(pcm, seed=seed, config=config)` applies to a batch of B clips: float32 [B, 48] on the device,
    8 x [b0, b1, b2, a1, a2], the drive d, 7 zeros per clip (ww_channel_draw).  Clip c's record does not depend on B."""
    if B < 0:
        raise ValueError(f"channel_records: B = {B}")
    g = _channel_struct(config)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"channel_records on {device}: this path has no CPU implementation")
    records = torch.empty((B, nat.CHANNEL_RECORD_F32), device=device, dtype=torch.float32)
    with torch.cuda.device(device):
        nat.check(nat.lib.ww_channel_draw(int(seed) & (2 ** 64 - 1), B, C.byref(g), _ptr(records), _stream()))
    return records


def channel_coefficients(kind: str, hz: float, db: float = 0.0, q: float = 2.0 ** -0.5):
    """One second-order section of the RBJ "Audio EQ Cookbook" at 16 kHz in numpy float64: (b0, b1, b2, a1, a2), divided by a0.
    kind: "highpass", "lowpass", "peak", "low_shelf", "high_shelf"; the shelves take q as their slope's Q."""
    w0 = 2.0 * np.pi * np.float64(hz) / 16000.0
    cs, alpha = np.cos(w0), np.sin(w0) / (2.0 * np.float64(q))
    A = np.power(np.float64(10.0), np.float64(db) / 40.0)
    if kind == "highpass":
        b, a = ((1.0 + cs) / 2.0, -(1.0 + cs), (1.0 + cs) / 2.0), (1.0 + alpha, -2.0 * cs, 1.0 - alpha)
    elif kind == "lowpass":
        b, a = ((1.0 - cs) / 2.0, 1.0 - cs, (1.0 - cs) / 2.0), (1.0 + alpha, -2.0 * cs, 1.0 - alpha)
    elif kind == "peak":
        b, a = (1.0 + alpha * A, -2.0 * cs, 1.0 - alpha * A), (1.0 + alpha / A, -2.0 * cs, 1.0 - alpha / A)
    elif kind in ("low_shelf", "high_shelf"):
        t, ap, am = 2.0 * np.sqrt(A) * alpha, A + 1.0, A - 1.0
        if kind == "low_shelf":
            b = (A * (ap - am * cs + t), 2.0 * A * (am - ap * cs), A * (ap - am * cs - t))
            a = (ap + am * cs + t, -2.0 * (am + ap * cs), ap + am * cs - t)
        else:
            b = (A * (ap + am * cs + t), -2.0 * A * (am + ap * cs), A * (ap + am * cs - t))
            a = (ap - am * cs + t, 2.0 * (am - ap * cs), ap - am * cs - t)
    else:
        raise ValueError(f"channel_coefficients: unknown section kind {kind!r}")
    return np.array([b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]], dtype=np.float64)


def pack_channel_plans(plans) -> np.ndarray:
    """A list of dicts, one per clip -> numpy float32 [B, 48] in the kernel's record layout.  Keys, all optional: "highpass": hz,
    "low_shelf": (hz, db), "peaks": [(hz, db, q), ...] (at most 4), "high_shelf": (hz, db), "lowpass": hz, "drive": d.  A missing key is
    an identity section (no saturator).  The coefficients are computed in numpy float64 (channel_coefficients) and rounded once.
    ValueError for a frequency outside (0, 7600], a Q <= 0, more than 4 peaks or a drive outside [0, 8]."""
    out = np.zeros((len(plans), nat.CHANNEL_RECORD_F32), dtype=np.float32)
    out[:, 0:5 * CHANNEL_SECTIONS:5] = 1.0

    def hz_of(i, v):
        v = float(v)
        if not 0.0 < v <= CHANNEL_MAX_HZ:
            raise ValueError(f"plan {i}: frequency {v} outside (0, {CHANNEL_MAX_HZ:g}] Hz")
        return v

    for i, plan in enumerate(plans):
        unknown = set(plan) - {"highpass", "low_shelf", "peaks", "high_shelf", "lowpass", "drive"}
        if unknown:
            raise ValueError(f"plan {i}: unknown keys {sorted(unknown)}")
        sections = {}
        if plan.get("highpass") is not None:
            sections[0] = channel_coefficients("highpass", hz_of(i, plan["highpass"]))
        if plan.get("low_shelf") is not None:
            sections[1] = channel_coefficients("low_shelf", hz_of(i, plan["low_shelf"][0]), float(plan["low_shelf"][1]))
        peaks = list(plan.get("peaks") or ())
        if len(peaks) > CHANNEL_MAX_PEAKS:
            raise ValueError(f"plan {i}: {len(peaks)} peaks; a record holds {CHANNEL_MAX_PEAKS}")
        for k, (hz, db, q) in enumerate(peaks):
            if not float(q) > 0.0:
                raise ValueError(f"plan {i}: peak Q {q} <= 0")
            sections[2 + k] = channel_coefficients("peak", hz_of(i, hz), float(db), float(q))
        if plan.get("high_shelf") is not None:
            sections[6] = channel_coefficients("high_shelf", hz_of(i, plan["high_shelf"][0]), float(plan["high_shelf"][1]))
        if plan.get("lowpass") is not None:
            sections[7] = channel_coefficients("lowpass", hz_of(i, plan["lowpass"]))
        for slot, co in sections.items():
            out[i, 5 * slot:5 * slot + 5] = co.astype(np.float32)
        d = float(plan.get("drive") or 0.0)
        if not 0.0 <= d <= CHANNEL_MAX_DRIVE:
            raise ValueError(f"plan {i}: drive {d} outside [0, {CHANNEL_MAX_DRIVE:g}]")
        out[i, 5 * CHANNEL_SECTIONS] = d
    return out


def _require_channel_pcm(pcm) -> None:
    if not isinstance(pcm, torch.Tensor):
        raise TypeError(f"pcm: expected a torch.Tensor, got {type(pcm).__name__}")
    if pcm.device.type != "cuda":
        raise RuntimeError(f"pcm is on {pcm.device}: this path has no CPU implementation; move it to the MI355X (`.cuda()`)")
    if pcm.dtype != torch.float32 or pcm.dim() != 2 or not pcm.is_contiguous():
        raise ValueError(f"pcm: expected contiguous float32 [B, N], got {pcm.dtype} {tuple(pcm.shape)}")
    if not CHANNEL_MIN_SAMPLES <= pcm.shape[1] <= CHANNEL_MAX_SAMPLES:
        raise NotImplementedError(f"pcm: {pcm.shape[1]} samples per clip; the channel stage takes {CHANNEL_MIN_SAMPLES}..{CHANNEL_MAX_SAMPLES} "
                                  "(the lengths augmentation runs at)")


def channel_effects(pcm: torch.Tensor, records=None, *, seed=None, config=ChannelConfig, out=None) -> torch.Tensor:
    """pcm float32 [B, N] on the GPU, contiguous, N = 4000 .. 16383 -> the same shape, every clip through its record's second-order
    sections and saturator.  Exactly one of `records` (float32 [B, 48] on the device: channel_records, or pack_channel_plans uploaded)
    and `seed` (the records are drawn inside the kernel from `config`) is given.  `out=pcm` filters in place (a clip whose record is
    "off" is then neither read nor written); any other `out` is a contiguous tensor like pcm that does not overlap it."""
    _require_channel_pcm(pcm)
    B, N = int(pcm.shape[0]), int(pcm.shape[1])
    if (records is None) == (seed is None):
        raise ValueError("channel_effects: give exactly one of `records` and `seed`")
    g = None
    if records is not None:
        if (not isinstance(records, torch.Tensor) or records.dtype != torch.float32 or tuple(records.shape) != (B, nat.CHANNEL_RECORD_F32)
                or records.device != pcm.device):
            raise ValueError(f"records: expected float32 [{B}, {nat.CHANNEL_RECORD_F32}] on {pcm.device}")
        records = records.contiguous()
        if records.data_ptr() % 16:
            records = records.clone()
        seed = 0
    else:
        g = _channel_struct(config)
    if out is None:
        out = torch.empty_like(pcm)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.shape != pcm.shape or out.device != pcm.device
          or not out.is_contiguous()):
        raise ValueError("out: expected a contiguous float32 tensor of pcm's shape on pcm's device")
    with torch.cuda.device(pcm.device):
        nat.check(nat.lib.ww_channel_f32(_ptr(pcm), _ptr(out), B, N, N, None if records is None else _ptr(records), int(seed) & (2 ** 64 - 1),
                                         None if g is None else C.byref(g), _stream()))
    return out
