"""Streaming sliding-window detection: many microphones, one hop per step, hipGraph-replayed.

The reference has no streaming code; the per-window semantics are `predict_wakeword` (notebook cell 19,
wakeword_training.ipynb:871-893): peak-normalise the last N samples, log-mel, forward, softmax, p[1] >= 0.8.
The window is the model's clip length, N = int(16000 * DURATION) for DURATION in [0.25, 1] (T = 1 + N // 512 <= 32 frames: the
lengths the model trains at).  Per hop this keeps an N-sample ring per microphone in HBM, appends the hop, recomputes the whole window
(frames cannot be reused across 10 ms hops: the 512-sample STFT grid realigns only every 2560 samples and
`ref=np.max` is per window -- SURVEY.md section 7) and replays one captured hipGraph:
ring append -> K1 -> K2 -> K3 (+softmax).

Hops may also come at the microphone's own rate, sample format and channel count (`sample_rate`, `dtype`, `channels`): the graph's first
node then converts, mixes to mono and resamples the hop to 16 kHz with K0's filter (bit for bit what the file path computes for a
recording of the same frames), `latency_samples` 16 kHz samples behind the input.
"""
from __future__ import annotations

import ctypes as C
import numbers

import torch

from . import _native as nat
from .config import CLIP_SAMPLES, N_FRAMES

# hop dtypes and the K0 sample format each is read as
_FORMATS = {torch.float32: nat.FMT_F32, torch.int16: nat.FMT_S16}


class StreamingDetector:
    def __init__(self, model, n_mics: int = 256, hop_samples: int = 160, threshold: float = 0.8, device=None, *,
                 sample_rate: int = 16000, channels: int = 1, dtype: torch.dtype = torch.float32, smooth=None, refractory_s=None):
        """hop_samples counts input frames at `sample_rate`; `dtype` (float32, or int16 read as PCM-16) and `channels` (1 .. 8,
        interleaved) are the hop's.  The window, `prob`, `logits` and `detections()` are at 16 kHz whatever the input.
        `smooth` (windows, 1 .. 256) / `refractory_s` (seconds): with either set (the other then defaults to 1 window / 1.0 s, as in
        scan.Scan.events), every step also runs the event rule of INTEGRATION.md section 3f per microphone -- the mean of the last
        `smooth` probabilities (NaN counting as 0) against `threshold`, at most one event per refractory period -- and detections()
        returns its flags.  With both None, detections() is `prob >= threshold`."""
        if model.training:
            raise NotImplementedError("call model.eval() first")
        n = int(getattr(model, "_n_samples", CLIP_SAMPLES))
        if 1 + n // 512 > N_FRAMES:
            raise NotImplementedError(f"streaming runs windows of 0.25 .. 1 s (at most {N_FRAMES} frames); this model is built for clips "
                                      f"of {n} samples")
        self.window_samples = n                        # N: the window every hop is scored on
        self.sample_rate, self.channels, self.dtype = self._check_input(n, int(hop_samples), sample_rate, channels, dtype)
        self._events = smooth is not None or refractory_s is not None
        if self._events:
            from .scan import _check_smooth, refractory_windows
            self.smooth = _check_smooth(1 if smooth is None else smooth)
            self.refractory_s = 1.0 if refractory_s is None else refractory_s
            if not 0.0 < float(threshold) <= 1.0:
                raise ValueError(f"threshold {threshold!r}: events need 0 < threshold <= 1")
            self._refractory = refractory_windows(self.refractory_s, self._hop16(int(hop_samples), sample_rate))
        self._input = (self.sample_rate, self.dtype, self.channels) != (16000, torch.float32, 1)
        self.device = torch.device(device) if device is not None else model.fc.weight.device
        if self.device.type != "cuda":
            raise RuntimeError("StreamingDetector needs the model on the MI355X (no CPU path)")
        self.n_mics, self.hop, self.threshold = int(n_mics), int(hop_samples), float(threshold)
        self._packed = model.packed_weights()          # keep alive: the graph holds its pointer
        self._n_conv = model._n_conv
        self._stream = torch.cuda.Stream(device=self.device)
        shape = (self.n_mics, self.hop) if self.channels == 1 else (self.n_mics, self.hop, self.channels)
        self.hop_buf = torch.zeros(shape, device=self.device, dtype=self.dtype)
        self.prob = torch.zeros(self.n_mics, device=self.device, dtype=torch.float32)
        self.logits = torch.zeros((self.n_mics, 2), device=self.device, dtype=torch.float32)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            if self._input:
                nat.check(nat.lib.ww_streamer_create_input(self.n_mics, self.hop, self.sample_rate, _FORMATS[self.dtype], self.channels,
                                                           self.window_samples, C.c_void_p(self._packed.data_ptr()), self._n_conv,
                                                           C.c_void_p(self._stream.cuda_stream), C.byref(handle)))
            else:
                nat.check(nat.lib.ww_streamer_create_n(self.n_mics, self.hop, self.window_samples, C.c_void_p(self._packed.data_ptr()),
                                                       self._n_conv, C.c_void_p(self._stream.cuda_stream), C.byref(handle)))
        self._h = handle
        if self._events:
            self._ev_state = torch.zeros(nat.check(nat.lib.ww_events_state_bytes(self.n_mics, self.smooth)), device=self.device,
                                         dtype=torch.uint8)
            self._fired = torch.zeros(self.n_mics, device=self.device, dtype=torch.bool)
            self._stream.wait_stream(torch.cuda.current_stream(self.device))      # the zeroed state before the first step
        self.latency_samples = int(nat.lib.ww_streamer_latency(handle))   # D: the window lags the input by D samples at 16 kHz

    @staticmethod
    def _hop16(hop, sample_rate):
        """The hop in 16 kHz samples: one window per hop."""
        if int(sample_rate) == 16000:
            return max(1, hop)
        up, down = C.c_int32(), C.c_int32()
        nat.lib.ww_resample_taps_host(int(sample_rate), None, 0, C.byref(up), C.byref(down), None)
        return max(1, hop * up.value // down.value)

    @staticmethod
    def _check_input(n, hop, sample_rate, channels, dtype):
        """The input format, checked without a device: (sample_rate, channels, dtype) or TypeError / ValueError."""
        if dtype not in _FORMATS:
            raise TypeError(f"dtype {dtype}: hops are torch.float32 or torch.int16")
        for name, v in (("sample_rate", sample_rate), ("channels", channels)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral):
                raise TypeError(f"{name} must be an integer, got {type(v).__name__}")
        sample_rate, channels = int(sample_rate), int(channels)
        if not 1000 <= sample_rate <= 384000:
            raise ValueError(f"sample_rate {sample_rate}: expected 1000 .. 384000 Hz")
        if not 1 <= channels <= 8:
            raise ValueError(f"channels {channels}: expected 1 .. 8")
        if (sample_rate, dtype, channels) != (16000, torch.float32, 1):
            # the library's rule (ww_streamer_create_input), checked here so that a bad hop never reaches a device
            up, down = C.c_int32(), C.c_int32()
            nat.lib.ww_resample_taps_host(sample_rate, None, 0, C.byref(up), C.byref(down), None)
            out = hop * up.value // down.value
            if hop < 1 or hop * up.value % down.value or out < 4 or out % 4 or out > n or n % out:
                raise ValueError(f"hop_samples {hop} at {sample_rate} Hz: hop_samples * {up.value} / {down.value} samples at 16 kHz must "
                                 f"be a whole multiple of 4 that divides the window of {n}")
        return sample_rate, channels, dtype

    @property
    def stream(self) -> torch.cuda.Stream:
        return self._stream

    def step(self, hop: torch.Tensor | None = None) -> torch.Tensor:
        """Push one hop [n_mics, hop_samples] (or [n_mics, hop_samples, channels]; or reuse whatever is in `hop_buf`) and enqueue the
        graph.  Returns `self.prob` (softmax p(wakeword) per mic), valid once `self.stream` has caught up."""
        if hop is not None and self._input:
            if hop.dtype != self.dtype:
                raise TypeError(f"hop dtype {hop.dtype}: this detector takes {self.dtype}")
            if tuple(hop.shape) != tuple(self.hop_buf.shape):
                raise ValueError(f"hop shape {tuple(hop.shape)}: expected {tuple(self.hop_buf.shape)}")
        if hop is not None:
            if hop.device.type == "cuda":
                # `hop` was produced on the caller's stream: order our stream behind it before reading it
                self._stream.wait_stream(torch.cuda.current_stream(self.device))
                hop.record_stream(self._stream)
            with torch.cuda.stream(self._stream):
                self.hop_buf.copy_(hop, non_blocking=True)
        with torch.cuda.device(self.device):
            if self._input:
                nat.check(nat.lib.ww_streamer_step_input(self._h, C.c_void_p(self.hop_buf.data_ptr()), C.c_void_p(self.prob.data_ptr()),
                                                         C.c_void_p(self.logits.data_ptr())))
            else:
                nat.check(nat.lib.ww_streamer_step(self._h, C.c_void_p(self.hop_buf.data_ptr()), C.c_void_p(self.prob.data_ptr()),
                                                   C.c_void_p(self.logits.data_ptr())))
            if self._events:
                # its own launch on the detector's stream, after the graph replay (the captured graph is unchanged)
                nat.check(nat.lib.ww_events_step_f32(C.c_void_p(self.prob.data_ptr()), self.n_mics, self.smooth, C.c_float(self.threshold),
                                                     self._refractory, C.c_void_p(self._ev_state.data_ptr()),
                                                     C.c_void_p(self._fired.data_ptr()), C.c_void_p(self._stream.cuda_stream)))
        return self.prob

    def detections(self) -> torch.Tensor:
        self._stream.synchronize()
        if self._events:
            return self._fired.clone()
        return self.prob >= self.threshold

    def window(self) -> torch.Tensor:
        """Current window of every microphone, oldest sample first: [n_mics, window_samples]."""
        out = torch.empty((self.n_mics, self.window_samples), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            nat.check(nat.lib.ww_streamer_window(self._h, C.c_void_p(out.data_ptr())))
        self._stream.synchronize()
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._stream.synchronize()
            nat.lib.ww_streamer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
