"""Background noise bank: every noise file decoded whole and kept in device memory, for mixing into training clips at a random SNR.

The reference gathers background noise (notebook cell 13: `background_files = load_audio_files('background_noise')`;
`create_sample_data` writes 20 noise files, wakeword_training_script.py:381-388) and never uses it.  Here a processor with a bank
attached (`AudioProcessor.set_background_noise`) mixes a segment of a random file into each clip inside KA, after time-stretch and crop
and before the Gaussian noise, at an SNR drawn in [BACKGROUND_SNR_MIN, BACKGROUND_SNR_MAX] dB -- MS-SNSD's snr_mixer recipe with the SNR
as named ("Background noise").

Memory: 4 bytes per sample of 16 kHz audio (230 MB per hour of noise), one float32 buffer on the device; offsets and lengths are
int64, so a bank may hold more than 2^31 samples (37 h).
"""
from __future__ import annotations

import os
import time

import numpy as np
import torch

from .config import AudioConfig

AUDIO_EXTENSIONS = (".wav", ".flac")


def list_audio_files(directory):
    """The WAV and FLAC files directly under `directory`, sorted by name (the notebook's load_audio_files('background_noise'))."""
    return sorted(os.path.join(directory, f) for f in os.listdir(directory)
                  if f.lower().endswith(AUDIO_EXTENSIONS) and os.path.isfile(os.path.join(directory, f)))


class BackgroundNoiseBank:
    """`BackgroundNoiseBank(paths, device=None, max_seconds=None)`: decode every file whole -- native reader -> K0, mono mix, resample to
    16 kHz, no normalisation, no crop: each file's samples equal AudioProcessor.load_audio(path) bit for bit -- into one float32 device
    buffer.  The decoded samples never pass through the host.

      data      float32 device tensor [n_samples], the files back to back
      offsets   int64 ndarray [n_files]: a file's first sample in `data`
      lengths   int64 ndarray [n_files]: its samples (all > 0)
      skipped   files left out because they could not be read or held no samples
      stats     the build rate: files, seconds of audio, wall seconds, audio seconds per second, files per second

    `paths`: a list of files, or a directory (its WAV and FLAC files, sorted).  `max_seconds`: stop adding files, in list order, once the
    bank holds that much audio (the file that crosses the cap is kept whole).  Raises ValueError when no file is left.  The build uses a
    reader of its own, closed when it is done (never the processor's shared one, which a running loader may own)."""

    def __init__(self, paths, device=None, max_seconds=None):
        from .audio import decode_whole_file
        from .files import WavBatchReader
        if isinstance(paths, (str, os.PathLike)) and os.path.isdir(paths):
            paths = list_audio_files(paths)
        paths = [os.fspath(p) for p in paths]
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("BackgroundNoiseBank lives on the MI355X and no GPU is visible (no CPU fallback)")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        cap = None if max_seconds is None else float(max_seconds) * AudioConfig.SAMPLE_RATE
        t0 = time.perf_counter()
        parts, lengths, self.skipped, total = [], [], 0, 0
        rd = WavBatchReader(max_clips=1, max_raw_bytes=1 << 22, slots=3, device=self.device)
        events, last = [None] * rd.slots, [0]

        def before_read(slot):                       # the staging of a slot is rewritten only after the work that last read it
            if events[slot] is not None:
                events[slot].synchronize()
            last[0] = slot
        try:
            with torch.cuda.device(self.device):
                for p in paths:
                    if cap is not None and total >= cap:
                        break
                    try:
                        samples = decode_whole_file(rd, p, self.device, before_read)
                    except Exception:
                        samples = None
                    events[last[0]] = torch.cuda.Event()
                    events[last[0]].record()
                    if samples is None or samples.numel() == 0:
                        self.skipped += 1
                        continue
                    parts.append(samples)
                    lengths.append(int(samples.numel()))
                    total += lengths[-1]
                if not parts:
                    raise ValueError(f"BackgroundNoiseBank: none of {len(paths)} file(s) could be read ({self.skipped} skipped)")
                self.data = torch.cat(parts)
                parts.clear()
                torch.cuda.current_stream().synchronize()
        finally:
            rd.close()
        self._set_index(np.asarray(lengths, dtype=np.int64))
        wall = time.perf_counter() - t0
        secs = self.n_samples / AudioConfig.SAMPLE_RATE
        self.stats = {"files": self.n_files, "skipped": self.skipped, "audio_seconds": secs, "wall_seconds": wall,
                      "audio_seconds_per_second": secs / wall if wall > 0 else float("inf"),
                      "files_per_second": (self.n_files + self.skipped) / wall if wall > 0 else float("inf")}

    @classmethod
    def from_buffer(cls, data: torch.Tensor, lengths):
        """A bank over an existing float32 device buffer holding files of `lengths` samples back to back (no copy, no decode): noise
        prepared elsewhere, and tests."""
        if not isinstance(data, torch.Tensor) or data.dtype != torch.float32 or data.dim() != 1 or data.device.type != "cuda":
            raise ValueError("BackgroundNoiseBank.from_buffer: expected a 1-D float32 tensor on the GPU")
        lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        if lengths.size == 0 or (lengths <= 0).any() or int(lengths.sum()) > data.numel():
            raise ValueError("BackgroundNoiseBank.from_buffer: lengths must be positive and fit in the buffer")
        bank = cls.__new__(cls)
        bank.device, bank.data, bank.skipped, bank.stats = data.device, data.contiguous(), 0, None
        bank._set_index(lengths)
        return bank

    def _set_index(self, lengths):
        self.lengths = lengths
        self.offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)

    @property
    def n_files(self) -> int:
        return int(self.lengths.size)

    @property
    def n_samples(self) -> int:
        return int(self.lengths.sum())

    @property
    def nbytes(self) -> int:
        return int(self.data.numel()) * 4

    def file(self, i: int) -> torch.Tensor:
        """File i's samples (a view of the device buffer)."""
        o, n = int(self.offsets[i]), int(self.lengths[i])
        return self.data[o:o + n]

    def __len__(self):
        return self.n_files

    def __repr__(self):
        return (f"BackgroundNoiseBank({self.n_files} files, {self.n_samples / AudioConfig.SAMPLE_RATE:.1f} s, "
                f"{self.nbytes / 2**20:.1f} MiB on {self.device}, {self.skipped} skipped)")
