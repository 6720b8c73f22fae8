"""ClipBank: training clips kept in device memory, cut into batches by a HIP kernel.

`WakewordDataset.loader()` opens, reads, uploads and decodes every file again each epoch although only the crop and the augmentation
draws change.  A ClipBank decodes each file once (`audio.decode_whole_file`: the samples are `AudioProcessor.load_audio(path)` bit
for bit), keeps the float32 samples on the device (230 MB per hour of 16 kHz audio) and builds every later batch with one gather
launch per segment touched (`ww_bank_gather_f32`, csrc/ww_bank.hip): no file, no upload and no host thread after the build.  It also
takes what never was a file: the windows `Scan.hard_negatives` mined (`add_pcm`) and the decoded audio of a `Scan` (`add_recordings`).

Two kinds of entry:
  clip    one item per epoch; start = random.randint(0, len - N) if len > N else 0, zero pad on the right (pad_or_truncate's rule);
          divided by the WHOLE entry's peak, then cropped (process_audio_file's order, what K0 does for the file loader)
  stream  `windows_per_epoch` items per epoch (default ceil(len / N)), each with a start drawn by the same rule; divided by the
          WINDOW's own peak, an all-zero window staying zero -- what the detector does to every window of a long recording
"""
from __future__ import annotations

import ctypes as C
import os
import random
import time

import numpy as np
import torch

from . import _native as nat
from .audit import STATS_DTYPE, BankAudit, active_start_range, check_crop, top_db_ratio
from .config import AudioConfig, n_samples
from .sampling import balanced_order, check_positive_fraction

# struct ww_bank_item as a numpy record (include/wakeword_amd.h)
ITEM_DTYPE = np.dtype([("offset", "<i8"), ("length", "<i8"), ("start", "<i8"), ("peak", "<f4"), ("row", "<i4"), ("norm", "<i4"),
                       ("reserved", "<i4")])
assert ITEM_DTYPE.itemsize == C.sizeof(nat.BankItem)
NORMS = {None: nat.BANK_NORM_NONE, "entry": nat.BANK_NORM_ENTRY, "window": nat.BANK_NORM_WINDOW}
CLIP, STREAM = 0, 1


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def bank_peaks(data: torch.Tensor, offsets) -> torch.Tensor:
    """ww_bank_peaks_f32: max |x| (fmaxf fold from 0) of the entries `offsets[e] .. offsets[e + 1]` of the 1-D float32 device tensor
    `data` -> float32 device tensor [n_entries].  `offsets`: int64 [n + 1], host or device."""
    if not isinstance(data, torch.Tensor) or data.dtype != torch.float32 or data.dim() != 1 or data.device.type != "cuda" or not data.is_contiguous():
        raise ValueError("bank_peaks: expected a contiguous 1-D float32 tensor on the GPU")
    off = torch.as_tensor(offsets, dtype=torch.int64).reshape(-1).to(data.device).contiguous()
    if off.numel() < 1:
        raise ValueError("bank_peaks: offsets must hold n_entries + 1 values")
    n = off.numel() - 1
    peaks = torch.empty(max(1, n), device=data.device, dtype=torch.float32)
    with torch.cuda.device(data.device):
        nat.check(nat.lib.ww_bank_peaks_f32(_ptr(data), data.numel(), _ptr(off), n, _ptr(peaks),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return peaks[:n]


class ClipBank:
    """`ClipBank(processor)`: an empty bank for clips of the processor's N samples on the processor's device.

      add_files(paths, label)                       one clip entry per file (unreadable files: placeholders served as zeros)
      add_pcm(pcm [M, n], label)                    one clip entry per row, stored as given (mined windows)
      add_recordings(paths | Scan, label=0, windows_per_epoch=None)   stream entries
      ClipBank.from_dataset(ds) / ds.cache()        clip entries in ds.files order with ds.labels
      gather(entries, starts=None, normalize="entry")   -> [B, N] on the device: the kernel, exposed
      loader(batch_size, shuffle, drop_last, augment)   the drop-in for dataset.loader(); crop="active" keeps windows on the sound
      audit(top_db, clip_level)                     -> BankAudit: levels, clipping, non-finite samples, active extent, content hash

    The bank is a list of segments: one 1-D float32 device tensor each, its entries back to back; segments are never concatenated
    with each other, and a batch whose items touch k segments costs k gather launches into disjoint rows.  Per entry (numpy, host):
    `lengths`, `labels`, `peaks` (ww_bank_peaks_f32, once per segment), `ok` (False for placeholders), `kinds`, `windows`."""

    def __init__(self, processor):
        self.processor = processor
        self.n_samples = int(n_samples(processor.config))
        self.device = processor.device                       # None until the first segment when the processor has not picked one
        self.segments = []                                   # 1-D float32 tensors
        self._seg = np.zeros(0, np.int64)                    # per entry: its segment,
        self._off = np.zeros(0, np.int64)                    # its first sample there,
        self.lengths = np.zeros(0, np.int64)
        self.peaks = np.zeros(0, np.float32)
        self.labels = np.zeros(0, np.int64)
        self.ok = np.zeros(0, bool)
        self.kinds = np.zeros(0, np.int8)
        self.windows = np.zeros(0, np.int64)                 # items per epoch (1 for a clip)
        self._items = None
        self._audits = {}                                    # (top_db, clip_level) -> BankAudit, until a segment is added
        self.stats = {"files": 0, "unreadable": 0, "audio_seconds": 0.0, "wall_seconds": 0.0, "audio_seconds_per_second": 0.0,
                      "files_per_second": 0.0}

    # ---- building -------------------------------------------------------------------------------
    def _add_segment(self, data, lengths, kind, labels, ok=None, windows=None, offsets=None, peaks=None):
        lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        n = lengths.size
        if offsets is None:
            offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64) if n else np.zeros(0, np.int64)
        offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
        if (lengths < 0).any() or (n and (int((offsets + lengths).max()) > data.numel() or (offsets < 0).any())):
            raise ValueError("ClipBank: entries must lie inside their segment")
        if data.numel() == 0:                                # a segment of placeholders only: the kernel still wants a buffer
            data = torch.zeros(1, device=data.device, dtype=torch.float32)
        if self.device is None:
            self.device = data.device
        if peaks is None:
            if n and np.array_equal(offsets[1:], (offsets + lengths)[:-1]) and offsets[0] == 0:
                table = np.concatenate([offsets, [offsets[-1] + lengths[-1]]])
                peaks = bank_peaks(data, table).cpu().numpy()                        # once per segment, copied to the host once
            elif n:
                raise ValueError("ClipBank: the entries of a segment lie back to back")
            else:
                peaks = np.zeros(0, np.float32)
        s = len(self.segments)
        self.segments.append(data)
        labels = np.broadcast_to(np.asarray(labels, dtype=np.int64), (n,))
        ok = np.ones(n, bool) if ok is None else np.asarray(ok, bool)
        if windows is None:
            windows = np.ones(n, np.int64) if kind == CLIP else -(-lengths // self.n_samples)
        self._seg = np.concatenate([self._seg, np.full(n, s, np.int64)])
        self._off = np.concatenate([self._off, offsets])
        self.lengths = np.concatenate([self.lengths, lengths])
        self.peaks = np.concatenate([self.peaks, np.asarray(peaks, np.float32)])
        self.labels = np.concatenate([self.labels, labels])
        self.ok = np.concatenate([self.ok, ok])
        self.kinds = np.concatenate([self.kinds, np.full(n, kind, np.int8)])
        self.windows = np.concatenate([self.windows, np.asarray(windows, np.int64)])
        self._items = None
        self._audits = {}
        return range(self.n_entries - n, self.n_entries)

    def _decode(self, paths):
        """Every file whole through a reader of this call's own -> (one device tensor, lengths, ok)."""
        from .audio import decode_whole_file
        from .files import WavBatchReader
        dev = self.processor._dev()
        parts, lengths, ok = [], [], []
        rd = WavBatchReader(max_clips=1, max_raw_bytes=1 << 22, slots=3, device=dev)
        events, last = [None] * rd.slots, [0]

        def before_read(slot):                       # the staging of a slot is rewritten only after the work that last read it
            if events[slot] is not None:
                events[slot].synchronize()
            last[0] = slot
        try:
            with torch.cuda.device(dev):
                for p in paths:
                    good = True
                    try:
                        samples = decode_whole_file(rd, p, dev, before_read)
                    except Exception:
                        samples, good = None, False
                    events[last[0]] = torch.cuda.Event()
                    events[last[0]].record()
                    ok.append(good)
                    lengths.append(0 if samples is None else int(samples.numel()))
                    if samples is not None and samples.numel():
                        parts.append(samples)
                data = torch.cat(parts) if parts else torch.zeros(1, device=dev, dtype=torch.float32)
                parts.clear()
                torch.cuda.current_stream().synchronize()
        finally:
            rd.close()
        return data, np.asarray(lengths, np.int64), np.asarray(ok, bool)

    def _count(self, t0, files, lengths, unreadable):
        st = self.stats
        st["files"] += int(files)
        st["unreadable"] += int(unreadable)
        st["audio_seconds"] += float(np.sum(lengths)) / AudioConfig.SAMPLE_RATE
        st["wall_seconds"] += time.perf_counter() - t0
        w = st["wall_seconds"]
        st["audio_seconds_per_second"] = st["audio_seconds"] / w if w > 0 else float("inf")
        st["files_per_second"] = st["files"] / w if w > 0 else float("inf")

    def _paths(self, paths):
        if isinstance(paths, (str, os.PathLike)):
            raise ValueError("paths: expected a list of files, not one path")
        return [os.fspath(p) for p in paths]

    def add_files(self, paths, label):
        """One clip entry per file, decoded whole (its samples equal load_audio(path) bit for bit).  `label`: one int, or one per file.
        A file that cannot be decoded becomes a placeholder (length 0, ok False, served as zeros) so that entries keep matching the
        list.  Returns the new entries' indices (a range)."""
        paths = self._paths(paths)
        t0 = time.perf_counter()
        data, lengths, ok = self._decode(paths)
        r = self._add_segment(data, lengths, CLIP, label, ok)
        self._count(t0, len(paths), lengths, (~ok).sum())
        return r

    def add_pcm(self, pcm, label):
        """pcm [M, n] (device or host, n >= 1): each row a clip entry of n samples, stored as given -- where
        `Scan.hard_negatives(...)[0]` goes: the entry peak of an un-normalised window is its window peak, so a mined window is
        trained on exactly as the detector saw it."""
        t = torch.as_tensor(pcm, dtype=torch.float32)
        if t.dim() != 2 or t.shape[1] < 1:
            raise ValueError(f"add_pcm: expected [M, n] with n >= 1, got {tuple(t.shape)}")
        if t.device.type != "cuda":
            t = t.to(self.processor._dev())
        t0 = time.perf_counter()
        r = self._add_segment(t.contiguous().reshape(-1), np.full(t.shape[0], t.shape[1], np.int64), CLIP, label)
        self._count(t0, 0, [t.numel()], 0)
        return r

    def add_buffer(self, data, lengths, label=0, stream=False):
        """A segment over an existing 1-D float32 device tensor holding entries of `lengths` samples back to back from its start (no
        copy, no decode): clip entries, or stream entries with stream=True.  Audio prepared elsewhere, and tests."""
        if not isinstance(data, torch.Tensor) or data.dtype != torch.float32 or data.dim() != 1 or not data.is_contiguous():
            raise ValueError("add_buffer: expected a contiguous 1-D float32 tensor")
        t0 = time.perf_counter()
        r = self._add_segment(data, lengths, STREAM if stream else CLIP, label)
        self._count(t0, 0, lengths, 0)
        return r

    def add_recordings(self, source, label=0, windows_per_epoch=None):
        """Stream entries: a list of paths (decoded as in add_files), or a `Scan` made with keep_audio=True, whose `audio` tensor
        becomes the segment with no copy.  Each entry yields `windows_per_epoch` windows per epoch (default ceil(len / N); an empty or
        unreadable recording yields none)."""
        from .scan import Scan
        if windows_per_epoch is not None and (isinstance(windows_per_epoch, bool) or int(windows_per_epoch) != windows_per_epoch
                                              or windows_per_epoch < 0):
            raise ValueError(f"windows_per_epoch {windows_per_epoch!r}: expected None or an integer >= 0")
        t0 = time.perf_counter()
        if isinstance(source, Scan):
            if source.audio is None:
                raise ValueError("this Scan was made with keep_audio=False: it holds no audio")
            data, lengths, offsets, ok, files = source.audio, source.lengths, source.offsets, np.ones(source.lengths.size, bool), 0
        else:
            paths = self._paths(source)
            data, lengths, ok = self._decode(paths)
            offsets, files = None, len(paths)
        if windows_per_epoch is None:
            windows = -(-lengths // self.n_samples)
        else:
            windows = np.where(lengths > 0, int(windows_per_epoch), 0).astype(np.int64)
        r = self._add_segment(data, lengths, STREAM, label, ok, windows, offsets)
        self._count(t0, files, lengths if files else [0], (~ok).sum())
        return r

    @classmethod
    def from_dataset(cls, ds):
        """Clip entries in ds.files order with ds.labels, on ds.processor (what `ds.cache()` returns)."""
        bank = cls(ds.processor)
        bank.add_files(ds.files, ds.labels)
        return bank

    # ---- what it holds --------------------------------------------------------------------------
    @property
    def n_entries(self) -> int:
        return int(self.lengths.size)

    @property
    def n_items(self) -> int:
        return int(self.windows.sum())

    @property
    def nbytes(self) -> int:
        return 4 * sum(int(s.numel()) for s in self.segments)

    @property
    def hours(self) -> float:
        return float(self.lengths.sum()) / AudioConfig.SAMPLE_RATE / 3600.0

    @property
    def unreadable(self) -> int:
        return int((~self.ok).sum())

    def __len__(self):
        return self.n_items

    def __repr__(self):
        return (f"ClipBank({self.n_entries} entries in {len(self.segments)} segment(s), {self.n_items} items per epoch, "
                f"{self.hours * 3600:.1f} s, {self.nbytes / 2**20:.1f} MiB on {self.device}, {self.unreadable} unreadable)")

    def item_entries(self) -> np.ndarray:
        """The entry of every item of an epoch: the clip entries in insertion order, then each stream entry's windows in insertion order."""
        if self._items is None:
            clips = np.flatnonzero(self.kinds == CLIP)
            streams = np.flatnonzero(self.kinds == STREAM)
            self._items = np.concatenate([clips, np.repeat(streams, self.windows[streams])]).astype(np.int64)
        return self._items

    def entry_samples(self, e) -> torch.Tensor:
        """Entry e's samples: a view of its segment, on the device."""
        e = int(e)
        if not 0 <= e < self.n_entries:
            raise ValueError(f"entry {e} outside [0, {self.n_entries})")
        return self.segments[int(self._seg[e])][int(self._off[e]):int(self._off[e] + self.lengths[e])]

    # ---- audit ----------------------------------------------------------------------------------
    def audit(self, top_db=60.0, clip_level=0.999) -> BankAudit:
        """One pass over every segment on the device (ww_bank_audit_f32: one call per segment, one copy to the host) -> BankAudit.
        `top_db`: a frame is active when its energy lies within top_db of the entry's loudest frame (librosa.effects.trim's rule);
        `clip_level`: |x| at or above it counts as clipped.  The result is kept until a segment is added."""
        ratio = top_db_ratio(top_db)
        clip_level = float(np.float32(clip_level))
        if not clip_level > 0.0:
            raise ValueError(f"clip_level {clip_level!r}: expected > 0")
        key = (float(top_db), clip_level)
        if key not in self._audits:
            parts = []
            for s, data in enumerate(self.segments):
                e = np.flatnonzero(self._seg == s)
                if e.size == 0:
                    continue
                table = np.ascontiguousarray(np.concatenate([self._off[e], [self._off[e[-1]] + self.lengths[e[-1]]]]), dtype=np.int64)
                with torch.cuda.device(data.device):
                    off = torch.from_numpy(table).to(data.device)
                    out = torch.empty(e.size * STATS_DTYPE.itemsize, device=data.device, dtype=torch.uint8)
                    ws = torch.empty(max(256, nat.check(nat.lib.ww_bank_audit_workspace_bytes(data.numel(), e.size))), device=data.device,
                                     dtype=torch.uint8)
                    nat.check(nat.lib.ww_bank_audit_f32(_ptr(data), data.numel(), _ptr(off), table.ctypes.data, e.size, clip_level, ratio,
                                                        _ptr(out), _ptr(ws), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
                parts.append(out)
            if parts:
                stats = torch.cat(parts).cpu().numpy().view(STATS_DTYPE).copy()       # segments hold their entries in bank order
            else:
                stats = np.zeros(0, STATS_DTYPE)
            self._audits[key] = BankAudit(stats, self.lengths.copy(), self.n_samples, self.labels.copy(), self.ok.copy(), self.kinds.copy(),
                                          bank=self, top_db=top_db, clip_level=clip_level)
        return self._audits[key]

    # ---- use ------------------------------------------------------------------------------------
    def draw_starts(self, entries, crop=None) -> np.ndarray:
        """The window start of each item, in order, with python `random` (pad_or_truncate's rule): random.randint(0, len - N) where
        len > N, else 0 and no draw (placeholders have length 0).  crop="active": a clip entry's start is drawn from the range that
        keeps the window on its active region (audit.active_start_range over `self.audit()`); one draw per entry with len > N either
        way, and stream entries keep the uniform rule."""
        N = self.n_samples
        starts = np.zeros(len(entries), np.int64)
        lengths = self.lengths[entries]
        if check_crop(crop) is None:
            for i in np.flatnonzero(lengths > N):
                starts[i] = random.randint(0, int(lengths[i]) - N)
            return starts
        au = self.audit()
        clip = self.kinds[entries] == CLIP
        lo, hi = active_start_range(lengths, np.where(clip, au.active_start[entries], 0), np.where(clip, au.active_end[entries], 0), N)
        for i in np.flatnonzero(lengths > N):
            starts[i] = random.randint(int(lo[i]), int(hi[i]))
        return starts

    def gather(self, entries, starts=None, normalize="entry", out=None, rows=None) -> torch.Tensor:
        """Windows of N samples of the given entries -> [B, N] float32 on the device.  `starts` (default 0): window start in entry
        coordinates, -N <= start <= len; the samples outside the entry are zero.  `normalize`: "entry" (divide by the entry's peak),
        "window" (by the window's own; a silent window stays zero) or None -- one value, or one per item.  `out`: a 2-D float32 device
        tensor with unit column stride to write into, `rows` the output row of each item (default 0 .. B - 1, no row twice); rows not
        named and columns from N on are left as they are.  Bad arguments raise ValueError before any device call."""
        N = self.n_samples
        entries = np.asarray(entries)
        if entries.ndim != 1 or (entries.size and entries.dtype.kind not in "iu"):
            raise ValueError("gather: entries must be a 1-D list of integers")
        entries = entries.astype(np.int64)
        B = entries.size
        if B and (entries.min() < 0 or entries.max() >= self.n_entries):
            raise ValueError(f"gather: entry index outside [0, {self.n_entries})")
        if starts is None:
            starts = np.zeros(B, np.int64)
        starts = np.asarray(starts)
        if starts.shape != (B,) or (B and starts.dtype.kind not in "iu"):
            raise ValueError("gather: starts must hold one integer per entry")
        starts = starts.astype(np.int64)
        if B and ((starts < -N).any() or (starts > self.lengths[entries]).any()):
            raise ValueError(f"gather: a start lies outside [-{N}, len]")
        if isinstance(normalize, (list, tuple, np.ndarray)):
            if len(normalize) != B or any(k not in NORMS for k in normalize):
                raise ValueError('gather: normalize takes "entry", "window" or None per item')
            norms = np.array([NORMS[k] for k in normalize], np.int32)
        elif normalize in NORMS:
            norms = np.full(B, NORMS[normalize], np.int32)
        else:
            raise ValueError(f'gather: normalize {normalize!r}: expected "entry", "window" or None')
        if rows is None:
            rows = np.arange(B, dtype=np.int64)
        rows = np.asarray(rows)
        if rows.shape != (B,) or (B and rows.dtype.kind not in "iu"):
            raise ValueError("gather: rows must hold one integer per entry")
        n_rows = B if out is None else (out.shape[0] if isinstance(out, torch.Tensor) and out.dim() == 2 else -1)
        if out is not None and (n_rows < 0 or out.dtype != torch.float32 or out.shape[1] < N or out.stride(1) != 1 or out.stride(0) < N
                                or out.device != self.device):
            raise ValueError(f"gather: out must be a 2-D float32 tensor on {self.device} with at least {N} columns of unit stride")
        if B and (rows.min() < 0 or rows.max() >= n_rows or np.unique(rows).size != B):
            raise ValueError("gather: rows must lie inside out and name no row twice")
        return self._gather(entries, starts, norms, out, rows.astype(np.int64))

    def _gather(self, entries, starts, norms, out=None, rows=None):
        """One ww_bank_gather_f32 launch per segment touched, into disjoint rows of `out` (arguments already checked)."""
        N, B, dev = self.n_samples, len(entries), self.device
        if out is None:
            out = torch.empty((B, N), device=dev, dtype=torch.float32)
        if rows is None:
            rows = np.arange(B, dtype=np.int64)
        if B == 0:
            return out
        seg = self._seg[entries]
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for s in np.unique(seg):
                pick = np.flatnonzero(seg == s)
                items = np.zeros(pick.size, ITEM_DTYPE)
                e = entries[pick]
                items["offset"], items["length"], items["start"] = self._off[e], self.lengths[e], starts[pick]
                items["peak"], items["row"], items["norm"] = self.peaks[e], rows[pick], norms[pick]
                data = self.segments[int(s)]
                ws = torch.empty(max(256, nat.check(nat.lib.ww_bank_gather_workspace_bytes(pick.size))), device=dev, dtype=torch.uint8)
                nat.check(nat.lib.ww_bank_gather_f32(_ptr(data), data.numel(), items.ctypes.data, pick.size, N, _ptr(out), out.shape[0],
                                                     out.stride(0), _ptr(ws), stream))
        return out

    def loader(self, batch_size=16, shuffle=False, drop_last=False, augment=False, positive_fraction=None, crop=None, entries=None):
        """What `dataset.loader(batch_size, shuffle, drop_last)` is, fed from device memory: re-iterable, with len() and order(),
        yielding `(data [B,1,80,T], target [B,1])` on the device.  `augment=True` runs processor.augment_batch on every batch;
        `positive_fraction=f` fixes the share of wake-word items of every epoch, as in dataset.loader.  `crop="active"` draws the
        window of a clip entry longer than the clip around its active region (draw_starts), instead of uniformly.  `entries`: a
        boolean mask [n_entries] or a strictly increasing list of entry indices restricts the epoch to the items of those entries, in
        the same relative order -- len(), order(), positive_fraction and drop_last act on the subset; what a bank built from those
        entries alone would yield, bit for bit.  With the writable `labels` this is how what a ledger.ClipLedger found is dropped or
        relabelled without rebuilding the bank.  After every batch `loader.last_entries` names the bank entry of each row."""
        return BankLoader(self, batch_size, shuffle=shuffle, drop_last=drop_last, augment=augment, positive_fraction=positive_fraction,
                          crop=crop, entries=entries)

    def select_entries(self, entries) -> np.ndarray:
        """A boolean mask [n_entries] or a strictly increasing list of entry indices -> the indices (int64, ascending).  ValueError for a
        mask of another length, an index outside the bank, an order that is not strictly increasing or an empty selection."""
        sel = np.asarray(entries)
        if sel.ndim != 1:
            raise ValueError("entries: expected a boolean mask [n_entries] or a 1-D list of entry indices")
        if sel.dtype == bool:
            if sel.size != self.n_entries:
                raise ValueError(f"entries: a mask of {sel.size} values for a bank of {self.n_entries} entries")
            sel = np.flatnonzero(sel)
        elif sel.size and sel.dtype.kind not in "iu":
            raise ValueError("entries: expected a boolean mask [n_entries] or a 1-D list of entry indices")
        sel = sel.astype(np.int64)
        if sel.size == 0:
            raise ValueError("entries: the selection is empty")
        if sel.min() < 0 or sel.max() >= self.n_entries:
            raise ValueError(f"entries: an index lies outside [0, {self.n_entries})")
        if (np.diff(sel) <= 0).any():
            raise ValueError("entries: the indices must be strictly increasing")
        return sel


class BankLoader:
    """One epoch = the bank's items (ClipBank.item_entries), in order or in a fresh `torch.randperm` per epoch.  Per batch, in this order:
    the starts of its items in batch order (python `random`; `crop="active"` changes their range, not their number), the gather, `processor.augment_batch` when augmenting (which draws its
    plans), `processor.channel_effects_batch(pcm, inplace=True)` when augmenting with `processor.set_channel_effects` on (which draws its
    seed), `processor.mel_batch(pcm, normalize=False)`, `processor.spec_augment_batch(data, inplace=True)` when augmenting with
    `processor.set_spec_augment` on (which draws its seed), rows of placeholders set to 0.0 -- the draw order of the file loader, so a
    seeded epoch over the same files yields the same batches bit for bit.  `entries` (ClipBank.select_entries) keeps only the items of
    those entries.  `last_entries`: the bank entry of every row of the newest batch (host int64; -1 for a placeholder row, served as
    zeros), set before the batch is yielded -- what a ledger.ClipLedger scatters by; nothing on the device is spent on it.
    `last_labels`: the rows' own int64 labels [B] on the device.  When augmenting with `processor.set_mixup` on, `processor.mixup_plan`
    (which draws) and `processor.mixup_batch` run last of all: `target` is then float32 [B, 2] class probabilities and `last_entries` is
    -1 on every mixed row as well."""

    def __init__(self, bank, batch_size=16, shuffle=False, drop_last=False, augment=False, positive_fraction=None, crop=None, entries=None):
        if batch_size < 1:
            raise ValueError("batch_size must be positive")
        self.crop = check_crop(crop)
        self.positive_fraction = check_positive_fraction(positive_fraction, bool(shuffle))
        if augment:
            bank.processor._check_augment()
        self.bank, self.batch_size, self.shuffle, self.drop_last, self.augment = bank, int(batch_size), bool(shuffle), bool(drop_last), bool(augment)
        self.entries = None if entries is None else bank.select_entries(entries)
        self.last_entries = None
        self.last_labels = None           # the rows' own int64 labels [B] on the device (what `target` held before mixup)

    def item_entries(self) -> np.ndarray:
        """The entry of every item of this loader's epoch: the bank's, restricted to `entries`."""
        items = self.bank.item_entries()
        return items if self.entries is None else items[np.isin(items, self.entries)]

    def __len__(self):
        n = self.bank.n_items if self.entries is None else int(self.item_entries().size)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def order(self):
        """Item order of one epoch (a fresh permutation from torch's default generator when shuffling; with positive_fraction the
        class-balanced draw of sampling.balanced_order over the items' labels)."""
        n = self.bank.n_items if self.entries is None else int(self.item_entries().size)
        if self.positive_fraction is not None:
            idx = balanced_order(self.bank.labels[self.item_entries()], self.positive_fraction).tolist()
        else:
            idx = torch.randperm(n).tolist() if self.shuffle else list(range(n))
        return idx[: len(self) * self.batch_size] if self.drop_last else idx

    def __iter__(self):
        bank, proc = self.bank, self.bank.processor
        item_entries = self.item_entries()
        idx = np.asarray(self.order(), dtype=np.int64)
        window = np.where(bank.kinds == STREAM, nat.BANK_NORM_WINDOW, nat.BANK_NORM_ENTRY).astype(np.int32)
        for s in range(0, idx.size, self.batch_size):
            entries = item_entries[idx[s:s + self.batch_size]]
            starts = bank.draw_starts(entries) if self.crop is None else bank.draw_starts(entries, self.crop)
            pcm = bank._gather(entries, starts, window[entries])
            if self.augment:
                pcm = proc.augment_batch(pcm)
                if getattr(proc, "channel_effects", None) is not None:
                    proc.channel_effects_batch(pcm, inplace=True)
            data = proc.mel_batch(pcm, normalize=False)
            if self.augment and getattr(proc, "spec_augment", None) is not None:
                proc.spec_augment_batch(data, inplace=True)
            bad = ~bank.ok[entries]
            if bad.any():
                data[torch.from_numpy(bad).to(data.device)] = 0.0
            target = torch.from_numpy(bank.labels[entries]).to(data.device).unsqueeze(1)
            self.last_entries = np.where(bad, -1, entries).astype(np.int64)
            self.last_labels = target[:, 0]
            if self.augment and getattr(proc, "mixup", None) is not None:
                # mixup last of all: a mixed row is no longer one entry's clip, so the ledger skips it (-1)
                partner, lam = proc.mixup_plan(len(entries), bad=bad)
                data, target = proc.mixup_batch(data, self.last_labels, plan=(partner, lam))
                self.last_entries = np.where(lam != 1.0, -1, self.last_entries).astype(np.int64)
            yield data, target
