"""Long recordings: per-window scores, events, false accepts per hour and false-reject rate.

  scan_files(model, paths, hop_samples=160)   -> Scan: every file decoded whole, every window of it scored in place on the GPU
  Scan.events(threshold, smooth, refractory_s) -> per file, the windows that fire and their times
  Scan.counts(thresholds, ...)                 -> [n_files, n_thresholds] event counts (HIP sweep kernel)
  Scan.hard_negatives(threshold, ...)          -> the windows that fired, as PCM for a mining round
  det_curve(model, positives, negatives)       -> FA/h and FRR over many thresholds; .threshold_for(fa_per_hour)

Windows: a recording x of L samples at 16 kHz has K = ceil(L / H) windows; window k (1 .. K) is x[kH - N, kH) with zeros outside x --
what a 16 kHz float32 StreamingDetector holds after k hops of the file.  Its score is the head's softmax p(wakeword) of forward_pcm on
it (NaN for a silent window).  Smoothing over w windows, threshold and refractory period: csrc/ww_events.hip.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import numbers

import numpy as np
import torch

from . import _native as nat
from .config import AudioConfig

SAMPLE_RATE = AudioConfig.SAMPLE_RATE


def _ptr(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check_hop(hop, n):
    if isinstance(hop, bool) or not isinstance(hop, numbers.Integral):
        raise ValueError(f"hop_samples must be an integer, got {type(hop).__name__}")
    hop = int(hop)
    if hop < 4 or hop > n or hop % 4:
        raise ValueError(f"hop_samples {hop}: expected a multiple of 4 in 4 .. {n} (the model's window)")
    return hop


def _check_smooth(smooth):
    if isinstance(smooth, bool) or not isinstance(smooth, numbers.Integral) or not 1 <= int(smooth) <= 256:
        raise ValueError(f"smooth {smooth!r}: expected an integer number of windows in 1 .. 256")
    return int(smooth)


def refractory_windows(refractory_s, hop):
    """R = ceil(seconds * 16000 / H): the windows after an event in which no other event fires."""
    try:
        r = float(refractory_s)
    except (TypeError, ValueError):
        raise ValueError(f"refractory_s {refractory_s!r}: expected a number of seconds") from None
    if not math.isfinite(r) or r < 0:
        raise ValueError(f"refractory_s {refractory_s!r}: expected a finite number of seconds >= 0")
    R = math.ceil(r * SAMPLE_RATE / hop)
    if R > 1 << 30:
        raise ValueError(f"refractory_s {refractory_s!r}: more than 2^30 windows")
    return int(R)


def _check_thresholds(thresholds):
    t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if t.size < 1 or t.size > 65536:
        raise ValueError(f"thresholds: expected 1 .. 65536 values, got {t.size}")
    t32 = t.astype(np.float32)
    if not np.all(np.isfinite(t32)) or not np.all((t32 > 0) & (t32 <= 1)):
        raise ValueError("thresholds must lie in (0, 1]")
    return t32


class Scan:
    """Scores of every window of a set of recordings (scan_files).

      prob            float32 device tensor [sum K]: file i's windows at prob[window_offsets[i]:window_offsets[i + 1]]
      window_offsets  int64 ndarray [n_files + 1]
      audio           float32 device tensor: the decoded files back to back (None with keep_audio=False)
      offsets         int64 ndarray [n_files]: a file's first sample in `audio`
      lengths         int64 ndarray [n_files]: its samples at 16 kHz
      paths           the scored files; `unreadable` the ones that could not be decoded (no hours, no windows)
      hop, window     H and N in samples at 16 kHz;  hours: the scored audio in hours"""

    def __init__(self, prob, lengths, paths, unreadable, hop, window, audio, device):
        self.prob = prob
        self.lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)
        n_win = -(-self.lengths // hop)
        self.window_offsets = np.concatenate([[0], np.cumsum(n_win)]).astype(np.int64)
        self.paths, self.unreadable = list(paths), list(unreadable)
        self.hop, self.window = int(hop), int(window)
        self.audio = audio
        self.device = device
        self.hours = float(self.lengths.sum()) / SAMPLE_RATE / 3600.0
        self._seg_dev = None

    @property
    def n_files(self) -> int:
        return len(self.paths)

    def file_prob(self, i: int) -> torch.Tensor:
        return self.prob[int(self.window_offsets[i]):int(self.window_offsets[i + 1])]

    def _sweep(self, thresholds, smooth, refractory_s, fired: bool):
        smooth = _check_smooth(smooth)
        R = refractory_windows(refractory_s, self.hop)
        thr = _check_thresholds(thresholds)
        if fired and thr.size != 1:
            raise ValueError("per-window flags need exactly one threshold")
        n_files, n_win = self.n_files, int(self.window_offsets[-1])
        counts = torch.zeros((n_files, thr.size), device=self.device, dtype=torch.int64)
        flags = torch.zeros(max(1, n_win), device=self.device, dtype=torch.uint8) if fired else None
        if n_files == 0:
            return counts.cpu().numpy(), (flags[:0].cpu().numpy() if fired else None)
        with torch.cuda.device(self.device):
            if self._seg_dev is None:
                self._seg_dev = torch.from_numpy(self.window_offsets).to(self.device)
            thr_dev = torch.from_numpy(thr).to(self.device)
            ws = torch.empty(max(256, nat.check(nat.lib.ww_events_workspace_bytes(n_win))), device=self.device, dtype=torch.uint8)
            nat.check(nat.lib.ww_events_sweep_f32(_ptr(self.prob), _ptr(self._seg_dev), n_files, n_win, smooth, R, _ptr(thr_dev), int(thr.size),
                                                  _ptr(counts), _ptr(flags) if fired else None, _ptr(ws), ws.numel(), _stream()))
            c = counts.cpu().numpy()
            f = flags[:n_win].cpu().numpy() if fired else None
        return c, f

    def counts(self, thresholds, smooth: int = 1, refractory_s: float = 1.0) -> np.ndarray:
        """Events per file at each threshold: int64 ndarray [n_files, n_thresholds] (one sweep kernel launch for all of them)."""
        return self._sweep(thresholds, smooth, refractory_s, False)[0]

    def events(self, threshold: float, smooth: int = 1, refractory_s: float = 1.0):
        """Per file, (windows, times): the 1-based numbers k of the windows that fire (int64) and their times k * H / 16000 in seconds
        (float64), both numpy."""
        _, flags = self._sweep([threshold], smooth, refractory_s, True)
        out = []
        for i in range(self.n_files):
            a, b = int(self.window_offsets[i]), int(self.window_offsets[i + 1])
            k = np.flatnonzero(flags[a:b]).astype(np.int64) + 1
            out.append((k, k * self.hop / SAMPLE_RATE))
        return out

    def hard_negatives(self, threshold: float, smooth: int = 1, refractory_s: float = 1.0, max_windows=None):
        """The windows that fire, cut from the decoded audio (zeros outside the file, not normalised): (pcm float32 device tensor [M, N],
        file index int64 ndarray [M], time in seconds float64 ndarray [M]) -- input for AudioProcessor.mel_batch / augment_batch."""
        if self.audio is None:
            raise ValueError("this Scan was made with keep_audio=False: it holds no audio to cut windows from")
        if max_windows is not None and (isinstance(max_windows, bool) or not isinstance(max_windows, numbers.Integral) or max_windows < 0):
            raise ValueError(f"max_windows {max_windows!r}: expected None or an integer >= 0")
        ev = self.events(threshold, smooth, refractory_s)
        files = np.concatenate([np.full(k.size, i, np.int64) for i, (k, _) in enumerate(ev)] + [np.zeros(0, np.int64)])
        ks = np.concatenate([k for k, _ in ev] + [np.zeros(0, np.int64)])
        if max_windows is not None:
            files, ks = files[:int(max_windows)], ks[:int(max_windows)]
        N, H = self.window, self.hop
        if files.size == 0:
            return torch.zeros((0, N), device=self.device, dtype=torch.float32), files, ks * H / SAMPLE_RATE
        start = ks * H - N                                                    # first sample of the window in file coordinates
        idx = torch.from_numpy(start).to(self.device)[:, None] + torch.arange(N, device=self.device)[None, :]
        L = torch.from_numpy(self.lengths[files]).to(self.device)[:, None]
        base = torch.from_numpy(self.offsets[files]).to(self.device)[:, None]
        inside = (idx >= 0) & (idx < L)
        pcm = torch.where(inside, self.audio[torch.where(inside, base + idx, torch.zeros_like(idx))], torch.zeros((), device=self.device))
        return pcm, files, ks * H / SAMPLE_RATE


def scan_files(model, paths, hop_samples: int = 160, batch_size: int = 4096, device=None, keep_audio: bool = True) -> Scan:
    """Decode every file whole (WAV / FLAC, any rate and channel count -> 16 kHz mono, AudioProcessor.load_audio's samples) through a
    reader of its own, and score all its windows of the model's N samples every `hop_samples`, `batch_size` windows per forward, read in
    place from the zero-padded signal (no copy of the windows).  The next file is read on the host while the GPU works on this one.
    A file that cannot be decoded is listed in `unreadable` and scored not at all."""
    from .audio import decode_whole_file
    from .files import WavBatchReader
    if model.training:
        raise NotImplementedError("call model.eval() first")
    N = int(model._n_samples)
    H = _check_hop(hop_samples, N)
    if isinstance(batch_size, bool) or not isinstance(batch_size, numbers.Integral) or not 1 <= int(batch_size) <= 1 << 20:
        raise ValueError(f"batch_size {batch_size!r}: expected an integer in 1 .. 2^20")
    batch_size = int(batch_size)
    if isinstance(paths, (str, os.PathLike)):
        raise ValueError("paths: expected a list of files, not one path")
    paths = [os.fspath(p) for p in paths]
    dev = torch.device(device) if device is not None else model.fc.weight.device
    if dev.type != "cuda":
        raise RuntimeError("scan_files needs the model on the MI355X (no CPU path)")
    packed, n_conv = model.packed_weights(), model._n_conv
    probs, lengths, parts, scored, unreadable = [], [], [], [], []
    rd = WavBatchReader(max_clips=1, max_raw_bytes=1 << 22, slots=3, device=dev)
    events, last = [None] * rd.slots, [0]

    def before_read(slot):                       # a slot's staging is rewritten only after the work that last read it
        if events[slot] is not None:
            events[slot].synchronize()
        last[0] = slot
    try:
        with torch.cuda.device(dev):
            ws_bytes = nat.check(nat.lib.ww_forward_windows_workspace_bytes(batch_size, N, n_conv))
            ws = torch.empty(max(256, ws_bytes), device=dev, dtype=torch.uint8)
            logits = torch.empty((batch_size, 2), device=dev, dtype=torch.float32)
            for p in paths:
                try:
                    samples = decode_whole_file(rd, p, dev, before_read)
                except Exception:
                    unreadable.append(p)
                    continue
                finally:
                    events[last[0]] = torch.cuda.Event()
                    events[last[0]].record()
                L = 0 if samples is None else int(samples.numel())
                K = -(-L // H)
                prob = torch.empty(K, device=dev, dtype=torch.float32)
                if K:
                    sig = torch.zeros(K * H + N, device=dev, dtype=torch.float32)      # N zeros, x, zeros to the end of window K
                    sig[N:N + L] = samples
                    for b0 in range(0, K, batch_size):
                        nb = min(batch_size, K - b0)
                        row0 = C.c_void_p(sig.data_ptr() + 4 * H * (b0 + 1))       # window b0 + 1 starts at H * (b0 + 1)
                        nat.check(nat.lib.ww_forward_windows_f32(row0, nb, H, N, 1, _ptr(packed), n_conv, _ptr(ws), ws.numel(),
                                                                 _ptr(logits), C.c_void_p(prob.data_ptr() + 4 * b0), _stream()))
                probs.append(prob)
                lengths.append(L)
                scored.append(p)
                if keep_audio and samples is not None:
                    parts.append(samples)
            prob = torch.cat(probs) if probs else torch.zeros(0, device=dev, dtype=torch.float32)
            audio = None
            if keep_audio:
                audio = torch.cat(parts) if parts else torch.zeros(0, device=dev, dtype=torch.float32)
            torch.cuda.current_stream().synchronize()
    finally:
        rd.close()
    return Scan(prob, lengths, scored, unreadable, H, N, audio, dev)


class DetCurve(dict):
    """det_curve's result: a dict (thresholds, fa_per_hour, frr, negative_hours, n_positive, unreadable) with threshold_for()."""

    def threshold_for(self, fa_per_hour: float = 0.5):
        """The lowest threshold whose false accepts per hour are at most `fa_per_hour` (None if no threshold meets it); its FRR is
        then the lowest this curve offers at that target."""
        fa = np.asarray(self["fa_per_hour"])
        ok = np.flatnonzero(fa <= float(fa_per_hour))
        if ok.size == 0:
            return None
        t = np.asarray(self["thresholds"])
        return float(t[ok[np.argmin(t[ok])]])


def det_curve(model, positive_paths, negative_paths, thresholds=None, hop_samples: int = 160, smooth: int = 1,
              refractory_s: float = 1.0, batch_size: int = 4096) -> DetCurve:
    """FA/h and FRR at every threshold (default: 1,000 values 0.001, 0.002, .., 1.0).  FA/h = events on the negative files / their
    hours; FRR = the fraction of readable positive files with no event.  Unreadable files count nowhere and are listed."""
    thr = _check_thresholds(np.linspace(0.001, 1.0, 1000) if thresholds is None else thresholds)
    _check_smooth(smooth)
    pos = [os.fspath(p) for p in positive_paths]
    neg = [os.fspath(p) for p in negative_paths]
    refractory_windows(refractory_s, _check_hop(hop_samples, int(model._n_samples)))
    sp = scan_files(model, pos, hop_samples, batch_size, keep_audio=False)
    sn = scan_files(model, neg, hop_samples, batch_size, keep_audio=False)
    cp = sp.counts(thr, smooth, refractory_s)
    cn = sn.counts(thr, smooth, refractory_s)
    hours = sn.hours
    with np.errstate(invalid="ignore", divide="ignore"):
        fa = cn.sum(axis=0) / hours if hours > 0 else np.full(thr.size, np.nan)
        frr = (cp == 0).sum(axis=0) / sp.n_files if sp.n_files else np.full(thr.size, np.nan)
    return DetCurve(thresholds=thr, fa_per_hour=np.asarray(fa, dtype=np.float64), frr=np.asarray(frr, dtype=np.float64), negative_hours=hours,
                    n_positive=sp.n_files, unreadable=sp.unreadable + sn.unreadable)


def threshold_for(curve, fa_per_hour: float = 0.5):
    """DetCurve.threshold_for for a plain dict of det_curve's keys."""
    return DetCurve(curve).threshold_for(fa_per_hour)
