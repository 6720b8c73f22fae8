"""Room impulse response bank: every RIR file decoded whole, trimmed around its direct path and kept on the device as a spectrum, for
reverberating training clips (far-field robustness).

A processor with a bank attached (`AudioProcessor.set_room_impulse_responses`) convolves a clip with a random RIR inside KA, after
time-stretch and crop and before the background noise, with probability AugmentationConfig.RIR_PROB.  The convolution is advanced by the
RIR's direct-path delay (the keyword stays where it was) and the result is rescaled to the clip's energy (INTEGRATION.md,
"Reverberation").  `ops.reverb` applies one RIR per clip on its own, for reverberant evaluation sets.

Trimming: d = the first index of max |h|; s = max(0, d - 40); the kept taps are h[s : s + min(len - s, 16384)], the direct path sits at
dpos = d - s.

Memory: only the spectra are kept, 16,385 complex float32 bins (128 KiB) per RIR: about 1.3 GB for 10,000 RIRs.
"""
from __future__ import annotations

import ctypes as C
import os
import time

import numpy as np
import torch

from . import _native as nat
from .background import list_audio_files
from .config import AudioConfig

MAX_TAPS = nat.RIR_MAX_TAPS          # 16384 taps kept at most (1.02 s at 16 kHz)
PRE_DIRECT = 40                      # taps kept before the direct path (2.5 ms)
SPECTRUM_BINS = nat.RIR_SPECTRUM_BINS


def trim_bounds(h):
    """The trimming rule on a 1-D array of taps (numpy or torch, host or device) -> (s, length, dpos): the kept taps are
    h[s : s + length] and the direct path sits at dpos within them.  The caller has rejected empty, all-zero and non-finite input."""
    a = h.abs() if isinstance(h, torch.Tensor) else np.abs(np.asarray(h))
    if isinstance(a, torch.Tensor):
        d = int(torch.nonzero(a == a.max())[0, 0])
    else:
        d = int(np.argmax(a))
    s = max(0, d - PRE_DIRECT)
    return s, min(int(a.shape[0]) - s, MAX_TAPS), d - s


class ImpulseResponseBank:
    """`ImpulseResponseBank(paths, device=None)`: decode every file whole -- native reader -> K0, mono mix, resample to 16 kHz, no
    normalisation: each file's samples equal AudioProcessor.load_audio(path) -- trim it (trim_bounds) and keep the spectrum of the kept
    taps zero-padded to 32,768 points, computed on the GPU.  The decoded samples never pass through the host.

      spectra   float32 device tensor [n_rirs, 16385, 2] (the library's bin order)
      dpos      int64 ndarray [n_rirs]: the direct path within the kept taps
      lengths   int64 ndarray [n_rirs]: the kept taps (1 .. 16384)
      skipped   files left out because they could not be read, or held no samples, only zeros or a non-finite value
      stats     the build rate: files, wall seconds, files per second

    `paths`: a list of files, or a directory (its WAV and FLAC files, sorted).  Raises ValueError when no file is left.  The build uses a
    reader of its own, closed when it is done."""

    def __init__(self, paths, device=None):
        from .audio import decode_whole_file
        from .files import WavBatchReader
        if isinstance(paths, (str, os.PathLike)) and os.path.isdir(paths):
            paths = list_audio_files(paths)
        paths = [os.fspath(p) for p in paths]
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("ImpulseResponseBank lives on the MI355X and no GPU is visible (no CPU fallback)")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        t0 = time.perf_counter()
        taps, self.skipped = [], 0
        rd = WavBatchReader(max_clips=1, max_raw_bytes=1 << 22, slots=3, device=self.device)
        try:
            with torch.cuda.device(self.device):
                for p in paths:
                    try:
                        h = decode_whole_file(rd, p, self.device)
                        torch.cuda.current_stream().synchronize()     # the reader's slot is free again before the next read
                    except Exception:
                        h = None
                    if h is None or h.numel() == 0 or not bool(torch.isfinite(h).all()) or not bool((h != 0).any()):
                        self.skipped += 1
                        continue
                    taps.append(h)
        finally:
            rd.close()
        if not taps:
            raise ValueError(f"ImpulseResponseBank: none of {len(paths)} file(s) could be used ({self.skipped} skipped)")
        self._build(taps)
        wall = time.perf_counter() - t0
        self.stats = {"files": self.n_rirs, "skipped": self.skipped, "wall_seconds": wall,
                      "files_per_second": (self.n_rirs + self.skipped) / wall if wall > 0 else float("inf")}

    @classmethod
    def from_taps(cls, taps, device=None):
        """A bank from RIRs already decoded (1-D arrays or tensors of taps at 16 kHz), trimmed by the same rule: simulated RIRs, and tests.
        Raises ValueError for an empty, all-zero or non-finite RIR."""
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        bank = cls.__new__(cls)
        bank.device, bank.skipped, bank.stats = torch.device(device), 0, None
        hs = []
        for i, h in enumerate(taps):
            t = torch.as_tensor(np.asarray(h, dtype=np.float32) if not isinstance(h, torch.Tensor) else h, dtype=torch.float32)
            t = t.reshape(-1).to(bank.device)
            if t.numel() == 0 or not bool(torch.isfinite(t).all()) or not bool((t != 0).any()):
                raise ValueError(f"ImpulseResponseBank.from_taps: RIR {i} is empty, all zero or not finite")
            hs.append(t)
        if not hs:
            raise ValueError("ImpulseResponseBank.from_taps: no RIR")
        bank._build(hs)
        return bank

    def _build(self, hs):
        """Trim every RIR, pack the kept taps into one device buffer and compute their spectra (ww_rir_spectra_f32)."""
        kept, dpos, lengths = [], [], []
        for h in hs:
            s, n, d = trim_bounds(h)
            kept.append(h[s:s + n])
            dpos.append(d)
            lengths.append(n)
        self.dpos = np.asarray(dpos, dtype=np.int64)
        self.lengths = np.asarray(lengths, dtype=np.int64)
        offsets = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)
        lens32 = self.lengths.astype(np.int32)
        with torch.cuda.device(self.device):
            buf = torch.cat(kept).contiguous()
            self.spectra = torch.empty((len(kept), SPECTRUM_BINS, 2), device=self.device, dtype=torch.float32)
            ws = torch.empty(max(1, nat.check(nat.lib.ww_rir_spectra_workspace_bytes(len(kept)))), device=self.device, dtype=torch.uint8)
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            nat.check(nat.lib.ww_rir_spectra_f32(C.c_void_p(buf.data_ptr()), buf.numel(), C.c_void_p(offsets.ctypes.data),
                                                 C.c_void_p(lens32.ctypes.data), len(kept), C.c_void_p(self.spectra.data_ptr()),
                                                 C.c_void_p(ws.data_ptr()), stream))
            torch.cuda.current_stream().synchronize()

    @property
    def n_rirs(self) -> int:
        return int(self.lengths.size)

    @property
    def nbytes(self) -> int:
        return int(self.spectra.numel()) * 4

    def __len__(self):
        return self.n_rirs

    def __repr__(self):
        return (f"ImpulseResponseBank({self.n_rirs} RIRs, {self.nbytes / 2**20:.1f} MiB of spectra on {self.device}, "
                f"{self.skipped} skipped)")
