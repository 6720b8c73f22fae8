"""BankAudit: what is in a ClipBank, measured on the device.

`ClipBank.audit()` runs `ww_bank_audit_f32` (csrc/ww_bank_audit.hip) once per segment and copies one record per entry to the host.  The
fields -- sums, clipped and non-finite counts, the content hash and the active extent -- are defined once, in include/wakeword_amd.h at
`ww_bank_audit_f32`; this module only derives from them: levels in dB, the flags of a policy, duplicate groups, a report, and the window
starts that `crop="active"` draws from (`active_start_range`, a pure function of lengths and extents)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as nat

# struct ww_bank_entry_stats as a numpy record (include/wakeword_amd.h)
STATS_DTYPE = np.dtype([("sum", "<f8"), ("sumsq", "<f8"), ("max_frame_energy", "<f8"), ("active_start", "<i8"), ("active_end", "<i8"),
                        ("hash", "<u8"), ("clipped", "<i8"), ("nonfinite", "<i8"), ("peak", "<f4"), ("reserved", "<i4")])
assert STATS_DTYPE.itemsize == C.sizeof(nat.BankEntryStats) == 72
CROPS = (None, "active")
FLAG_NAMES = ("unreadable", "empty", "silent", "clipped", "dc_offset", "short", "overlong", "nonfinite")


def check_crop(crop):
    if crop not in CROPS:
        raise ValueError(f'crop {crop!r}: expected None or "active"')
    return crop


def top_db_ratio(top_db) -> float:
    """The energy ratio below the loudest frame at which a frame stops counting as active: 10 ** (-top_db / 10), in (0, 1]."""
    top_db = float(top_db)
    if not (top_db >= 0.0) or top_db == float("inf"):
        raise ValueError(f"top_db {top_db!r}: expected a finite value >= 0")
    ratio = 10.0 ** (-top_db / 10.0)
    if not (0.0 < ratio <= 1.0):
        raise ValueError(f"top_db {top_db!r}: the energy ratio underflows")
    return ratio


def active_start_range(lengths, a, b, n):
    """The inclusive range (lo, hi) that the window start of each entry is drawn from under crop="active", for entries of `lengths`
    samples whose active extent is [a, b) and windows of `n` samples:

        len <= n                     (0, 0): the window starts at 0 and nothing is drawn
        len > n, b <= a              (0, len - n): no activity (or none known), the uniform window of pad_or_truncate
        len > n, b - a <= n          (max(0, b - n), min(a, len - n)): the window holds the whole active region
        len > n, b - a >  n          (a, b - n): the window lies inside the active region

    An entry with non-finite samples carries the extent (0, len) and so falls under the last row as (0, len - n), the uniform window."""
    lengths, a, b = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (lengths, a, b))
    n = int(n)
    if not (lengths.shape == a.shape == b.shape):
        raise ValueError("active_start_range: lengths, a and b must have one value per entry")
    if n < 1 or (lengths < 0).any() or (a < 0).any() or (b > np.maximum(lengths, 0)).any() or ((b > a) & (a >= lengths)).any():
        raise ValueError("active_start_range: expected n >= 1, lengths >= 0 and extents inside their entries")
    long = lengths > n
    none = b <= a
    fits = ~none & (b - a <= n)
    lo = np.where(fits, np.maximum(0, b - n), np.where(none, 0, a))
    hi = np.where(fits, np.minimum(a, lengths - n), np.where(none, lengths - n, b - n))
    return np.where(long, lo, 0).astype(np.int64), np.where(long, hi, 0).astype(np.int64)


class BankFlags:
    """Boolean arrays per entry, one per name in FLAG_NAMES, and `any`."""

    def __init__(self, **arrays):
        for k in FLAG_NAMES:
            setattr(self, k, np.asarray(arrays[k], bool))

    @property
    def any(self):
        out = np.zeros_like(self.empty)
        for k in FLAG_NAMES:
            out |= getattr(self, k)
        return out

    def counts(self):
        return {k: int(getattr(self, k).sum()) for k in FLAG_NAMES}


class BankAudit:
    """Per entry (numpy, host): `length`, `peak`, `rms_db`, `dc`, `crest_db`, `clipped`, `nonfinite`, `active_start`, `active_end`, `hash`,
    and the raw `sum`, `sumsq`, `max_frame_energy`; `labels`, `ok`, `kinds` copied from the bank.  rms_db and crest_db are dB (rms_db
    relative to full scale 1.0, -inf for a silent or empty entry; crest_db = peak over rms, nan where there is no rms).  `n_samples`:
    the clip length the bank serves.  Built by `ClipBank.audit()`, or from arrays (`BankAudit.from_stats`)."""

    def __init__(self, stats, lengths, n_samples, labels=None, ok=None, kinds=None, bank=None, top_db=60.0, clip_level=0.999):
        stats = np.asarray(stats)
        if stats.dtype != STATS_DTYPE or stats.ndim != 1:
            raise ValueError("BankAudit: stats must be a 1-D array of STATS_DTYPE")
        n = stats.size
        self.stats = stats
        self.length = np.asarray(lengths, np.int64).reshape(-1)
        if self.length.size != n:
            raise ValueError("BankAudit: one length per entry")
        self.n_samples = int(n_samples)
        self.labels = np.zeros(n, np.int64) if labels is None else np.asarray(labels, np.int64).reshape(-1)
        self.ok = np.ones(n, bool) if ok is None else np.asarray(ok, bool).reshape(-1)
        self.kinds = np.zeros(n, np.int8) if kinds is None else np.asarray(kinds, np.int8).reshape(-1)
        self.bank, self.top_db, self.clip_level = bank, float(top_db), float(clip_level)
        self.sum, self.sumsq, self.max_frame_energy = stats["sum"], stats["sumsq"], stats["max_frame_energy"]
        self.peak = stats["peak"]
        self.clipped, self.nonfinite = stats["clipped"], stats["nonfinite"]
        self.active_start, self.active_end, self.hash = stats["active_start"], stats["active_end"], stats["hash"]
        count = np.maximum(self.length - self.nonfinite, 1).astype(np.float64)      # sum and sumsq run over the finite samples
        with np.errstate(divide="ignore", invalid="ignore"):
            self.dc = self.sum / count
            rms = np.sqrt(self.sumsq / count)
            self.rms_db = np.where(rms > 0, 20.0 * np.log10(rms), -np.inf)
            self.crest_db = np.where(rms > 0, 20.0 * np.log10(self.peak.astype(np.float64) / rms), np.nan)

    @classmethod
    def from_stats(cls, lengths, n_samples, **fields):
        """An audit from hand-made arrays: any of STATS_DTYPE's fields by name (the rest zero), plus labels / ok / kinds / bank."""
        lengths = np.asarray(lengths, np.int64).reshape(-1)
        stats = np.zeros(lengths.size, STATS_DTYPE)
        extra = {}
        for k, v in fields.items():
            if k in STATS_DTYPE.names:
                stats[k] = v
            else:
                extra[k] = v
        return cls(stats, lengths, n_samples, **extra)

    def __len__(self):
        return int(self.length.size)

    # ---- policy ---------------------------------------------------------------------------------
    def flags(self, silent_db=-60.0, clipped_fraction=1e-3, dc=0.01, min_active=0.2) -> BankFlags:
        """unreadable: a placeholder (ok False).  empty: readable, no samples.  nonfinite: holds a NaN or an Inf (the other level flags
        are then off: its numbers describe the finite samples only).  silent: rms_db < silent_db or no active frame.  clipped: more than
        `clipped_fraction` of the samples at or above the audit's clip_level.  dc_offset: |mean| > dc.  short: an active region of less
        than `min_active` seconds.  overlong: an active region longer than the clip, so the word cannot fit in one window.  The
        thresholds are policy, not measurements."""
        from .config import AudioConfig
        has = self.ok & (self.length > 0)
        nonfinite = has & (self.nonfinite > 0)
        level = has & ~nonfinite
        active = self.active_end - self.active_start
        silent = level & ((self.rms_db < silent_db) | (active <= 0))
        sounding = level & ~silent
        return BankFlags(unreadable=~self.ok, empty=self.ok & (self.length == 0), nonfinite=nonfinite, silent=silent,
                         clipped=level & (self.clipped > clipped_fraction * self.length), dc_offset=level & (np.abs(self.dc) > dc),
                         short=sounding & (active < min_active * AudioConfig.SAMPLE_RATE), overlong=sounding & (active > self.n_samples))

    def report(self, worst=5, **policy) -> str:
        """Plain text: the bank in one line, counts per flag and label, and per flag the `worst` entries by index."""
        from .config import AudioConfig
        f = self.flags(**policy)
        sr = AudioConfig.SAMPLE_RATE
        n = len(self)
        labels = sorted(set(self.labels.tolist()))
        lines = [f"bank audit: {n} entries, {float(self.length.sum()) / sr:.1f} s, clip {self.n_samples / sr:.3f} s, "
                 f"top_db {self.top_db:g}, clip_level {self.clip_level:g}",
                 "entries per label: " + ", ".join(f"{lab}: {int((self.labels == lab).sum())}" for lab in labels),
                 f"flagged: {int(f.any.sum())} of {n}"]
        # what makes an entry the worst of its flag, largest first
        severity = {"unreadable": np.zeros(n), "empty": np.zeros(n), "silent": -np.where(np.isfinite(self.rms_db), self.rms_db, -1e9),
                    "clipped": self.clipped / np.maximum(self.length, 1), "dc_offset": np.abs(self.dc),
                    "short": -(self.active_end - self.active_start).astype(np.float64),
                    "overlong": (self.active_end - self.active_start).astype(np.float64), "nonfinite": self.nonfinite.astype(np.float64)}
        for k in FLAG_NAMES:
            m = getattr(f, k)
            per = ", ".join(f"{lab}: {int((m & (self.labels == lab)).sum())}" for lab in labels)
            lines.append(f"  {k:<10} {int(m.sum()):>7}" + (f"   (label {per})" if m.any() else ""))
            idx = np.flatnonzero(m)
            idx = idx[np.argsort(-severity[k][idx], kind="stable")][:worst]
            for e in idx:
                lines.append(f"      entry {int(e)}: label {int(self.labels[e])}, {self.length[e] / sr:.3f} s, rms {self.rms_db[e]:.1f} dBFS, "
                             f"peak {float(self.peak[e]):.4f}, dc {self.dc[e]:+.4f}, clipped {int(self.clipped[e])}, "
                             f"non-finite {int(self.nonfinite[e])}, active {self.active_start[e] / sr:.3f}-{self.active_end[e] / sr:.3f} s")
        return "\n".join(lines)

    # ---- duplicates -----------------------------------------------------------------------------
    def _same(self, e, other, f):
        """Entry e of this audit's bank and entry f of `other`'s hold the same float32 bits (compared where the samples live)."""
        import torch
        x, y = self.bank.entry_samples(e), other.bank.entry_samples(f)
        if x.device != y.device:
            y = y.to(x.device)
        return x.numel() == y.numel() and bool(torch.equal(x.view(torch.int32), y.view(torch.int32)))

    def duplicates(self, verify=True, other=None):
        """Groups of non-empty entries with equal (length, hash).  Without `other`: a list of lists of entry indices (two or more
        each, ascending).  With `other`, the BankAudit of a second bank (train against validation): a list of `(entries, other_entries)`
        pairs that share content -- leakage; duplicates inside one bank are not reported then.  `verify=True` confirms every group by
        comparing the samples bit for bit, so that a hash collision cannot merge two different clips; it needs audits made by
        `ClipBank.audit()` (they know their bank)."""
        if verify and (self.bank is None or (other is not None and other.bank is None)):
            raise ValueError("duplicates(verify=True) needs audits made by ClipBank.audit(); pass verify=False for arrays alone")
        parts = [(self, 0)] + ([(other, 1)] if other is not None else [])
        groups = {}
        for au, side in parts:
            for e in np.flatnonzero((au.length > 0) & au.ok):
                groups.setdefault((int(au.length[e]), int(au.hash[e])), []).append((side, int(e)))
        out = []
        for members in groups.values():
            if len(members) < 2:
                continue
            classes = []                                  # with verify: split by content, each class led by its first member
            for side, e in members:
                for cl in classes:
                    s0, e0 = cl[0]
                    if not verify or (self, other)[s0]._same(e0, (self, other)[side], e):
                        cl.append((side, e))
                        break
                else:
                    classes.append([(side, e)])
            for cl in classes:
                mine = [e for side, e in cl if side == 0]
                theirs = [e for side, e in cl if side == 1]
                if other is None and len(mine) > 1:
                    out.append(mine)
                elif other is not None and mine and theirs:
                    out.append((mine, theirs))
        out.sort(key=lambda g: g[0] if other is None else g[0][0])
        return out
