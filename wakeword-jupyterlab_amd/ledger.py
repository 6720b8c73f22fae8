"""ClipLedger and LedgerReport: what training did to every single clip.

`bank.audit()` says what a ClipBank holds before training and `ClipReport` scores a model in aggregate; a ClipLedger is the dynamic
counterpart: per bank entry, when it was seen, whether it was classified right and how large the margin of its ASSIGNED class was, kept
as integers in device memory by one launch per batch (`ww_clip_ledger_update_f32`, csrc/ww_ledger.hip; the per-row contract is defined
once, in include/wakeword_amd.h).  The mean margin over training is the area under the margin: negative for likely label errors.  Its
spread marks ambiguous clips; right-then-wrong transitions between epochs are forgetting events.

`LedgerReport` is pure numpy -- no torch, no GPU -- so a report can be built, added and questioned anywhere."""
from __future__ import annotations

import warnings

import numpy as np

# struct ww_ledger_header / ww_ledger_entry as numpy records (include/wakeword_amd.h)
HEADER_FIELDS = ("n_entries", "updates", "rows", "skipped", "bad_entries", "bad_labels", "nonfinite", "reserved")
ENTRY_DTYPE = np.dtype([("sum_q", "<i8"), ("sum_q2", "<u8"), ("seen_epochs", "<u8"), ("wrong_epochs", "<u8"), ("seen", "<i4"),
                        ("correct", "<i4"), ("nonfinite", "<i4"), ("min_q", "<i4"), ("max_q", "<i4"), ("reserved", "<i4")])
assert ENTRY_DTYPE.itemsize == 56
HEADER_BYTES = 8 * len(HEADER_FIELDS)
Q_SCALE = 65536                     # a margin is kept in units of 2^-16 ...
Q_LIMIT = 64.0                      # ... clamped to +-64
MAX_EPOCHS = 64                     # the epoch bitmaps are 64 bits wide
FLAG_NAMES = ("unseen", "suspect", "never_learned", "forgotten", "nonfinite")
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


class LedgerReport:
    """A ledger on the host.  Raw, per entry: `sum_q`, `sum_q2`, `seen_epochs`, `wrong_epochs`, `seen`, `correct`, `nonfinite`, `min_q`,
    `max_q` (views of `entries`, an ENTRY_DTYPE array) and `header`, a dict of the header counters.  Derived, per entry:

      seen_finite    seen - nonfinite
      mean_margin    sum_q / (65536 seen_finite), the area under the margin in logit units; NaN where seen_finite is 0
      std_margin     the population deviation sqrt(max(0, n sum_q2 - sum_q^2)) / (65536 n), n = seen_finite, its numerator formed in
                     exact Python integers (n sum_q2 overflows int64); NaN where n is 0
      min_margin, max_margin   NaN where seen_finite is 0
      accuracy       correct / seen; NaN where seen is 0
      learned_epoch  the lowest epoch that is seen and not wrong; -1 if none
      forgetting     over the entry's seen epochs in ascending order, the adjacent pairs that go right then wrong
      never_learned  seen in some recorded epoch and wrong in every one of them (learned_epoch == -1)

    An epoch is "wrong" for an entry when ANY of its visits in that epoch was classified wrongly.  Visits made with epoch -1 (evaluation,
    epochs past the 64th) count in the sums and in seen / correct, and in no bitmap.  Build with `ops.read_clip_ledger`,
    `LedgerReport.from_buffer` or `LedgerReport.from_arrays`."""

    def __init__(self, header, entries):
        entries = np.asarray(entries)
        if entries.dtype != ENTRY_DTYPE or entries.ndim != 1:
            raise ValueError("LedgerReport: entries must be a 1-D array of ENTRY_DTYPE")
        self.header = {k: int(header.get(k, 0)) for k in HEADER_FIELDS}
        self.header["n_entries"] = int(entries.size)
        self.entries = entries
        for k in ENTRY_DTYPE.names:
            setattr(self, k, entries[k])
        self._derived = {}

    @classmethod
    def from_buffer(cls, words, n_entries):
        """The device buffer's bytes (any integer array or bytes-like of 64 + 56 n_entries bytes) -> a report.  The header must name
        `n_entries` records: anything else means the buffer was overwritten."""
        raw = np.frombuffer(np.ascontiguousarray(words).tobytes() if isinstance(words, np.ndarray) else bytes(words), np.uint8)
        n_entries = int(n_entries)
        if raw.size != HEADER_BYTES + ENTRY_DTYPE.itemsize * n_entries:
            raise ValueError(f"a ledger of {n_entries} entries has {HEADER_BYTES + ENTRY_DTYPE.itemsize * n_entries} bytes, got {raw.size}")
        head = raw[:HEADER_BYTES].view("<i8")
        header = dict(zip(HEADER_FIELDS, head.tolist()))
        if header["n_entries"] != n_entries:
            raise RuntimeError(f"the ledger's header names {header['n_entries']} entries, expected {n_entries}: was the buffer overwritten?")
        return cls(header, raw[HEADER_BYTES:].view(ENTRY_DTYPE).copy())

    @classmethod
    def from_arrays(cls, n_entries, header=None, **fields):
        """A report from hand-made arrays: any of ENTRY_DTYPE's fields by name; the rest as ww_clip_ledger_init leaves them."""
        entries = np.zeros(int(n_entries), ENTRY_DTYPE)
        entries["min_q"], entries["max_q"] = INT32_MAX, INT32_MIN
        for k, v in fields.items():
            if k not in ENTRY_DTYPE.names:
                raise ValueError(f"LedgerReport.from_arrays: {k!r} is not a field of a ledger entry")
            entries[k] = v
        return cls(header or {}, entries)

    def tobytes(self) -> bytes:
        """The ledger's buffer as the device holds it: the header, then the records."""
        return np.array([self.header[k] for k in HEADER_FIELDS], "<i8").tobytes() + self.entries.tobytes()

    def __len__(self):
        return int(self.entries.size)

    @property
    def n_entries(self) -> int:
        return int(self.entries.size)

    def __eq__(self, other):
        return isinstance(other, LedgerReport) and self.tobytes() == other.tobytes()

    __hash__ = None

    # ---- derived -------------------------------------------------------------------------------
    def _get(self, name, make):
        if name not in self._derived:
            self._derived[name] = make()
        return self._derived[name]

    @property
    def seen_finite(self):
        return self._get("seen_finite", lambda: self.seen.astype(np.int64) - self.nonfinite)

    def _per_finite(self, numerator):
        n = self.seen_finite
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(n > 0, np.asarray(numerator, np.float64) / (float(Q_SCALE) * np.maximum(n, 1)), np.nan)

    @property
    def mean_margin(self):
        # |sum_q| <= 2^31 visits x 2^22 = 2^53: exact in float64, so this is the correctly rounded quotient
        return self._get("mean_margin", lambda: self._per_finite(self.sum_q))

    @property
    def std_margin(self):
        def make():
            n = self.seen_finite.astype(object)
            num = n * self.sum_q2.astype(object) - self.sum_q.astype(object) ** 2           # exact Python integers
            root = np.array([float(max(0, v)) ** 0.5 for v in num], np.float64).reshape(num.shape)
            return self._per_finite(root)
        return self._get("std_margin", make)

    @property
    def min_margin(self):
        return self._get("min_margin", lambda: np.where(self.seen_finite > 0, self.min_q / float(Q_SCALE), np.nan))

    @property
    def max_margin(self):
        return self._get("max_margin", lambda: np.where(self.seen_finite > 0, self.max_q / float(Q_SCALE), np.nan))

    @property
    def accuracy(self):
        def make():
            with np.errstate(divide="ignore", invalid="ignore"):
                return np.where(self.seen > 0, self.correct / np.maximum(self.seen, 1).astype(np.float64), np.nan)
        return self._get("accuracy", make)

    @property
    def learned_epoch(self):
        def make():
            right = self.seen_epochs & ~self.wrong_epochs
            out = np.full(len(self), -1, np.int64)
            for b in range(MAX_EPOCHS - 1, -1, -1):
                out[(right >> np.uint64(b)) & np.uint64(1) == 1] = b
            return out
        return self._get("learned_epoch", make)

    @property
    def forgetting(self):
        def make():
            count = np.zeros(len(self), np.int64)
            was_right = np.zeros(len(self), bool)                  # the newest seen epoch so far was right
            for b in range(MAX_EPOCHS):
                s = (self.seen_epochs >> np.uint64(b)) & np.uint64(1) == 1
                w = (self.wrong_epochs >> np.uint64(b)) & np.uint64(1) == 1
                count += s & w & was_right
                was_right = np.where(s, ~w, was_right)
            return count
        return self._get("forgetting", make)

    @property
    def never_learned(self):
        return self._get("never_learned", lambda: (self.seen_epochs != 0) & (self.learned_epoch == -1))

    # ---- policy --------------------------------------------------------------------------------
    def flags(self, min_seen=2) -> dict:
        """Boolean arrays per entry.  unseen: no visit.  suspect: at least `min_seen` finite visits and a negative mean margin -- the model
        kept voting against the label.  never_learned, forgotten (forgetting >= 1): as above.  nonfinite: a visit with a NaN or an
        infinite margin.  `min_seen` is policy, not measurement."""
        n = self.seen_finite
        with np.errstate(invalid="ignore"):
            suspect = (n >= int(min_seen)) & (n > 0) & (self.mean_margin < 0)
        return {"unseen": self.seen == 0, "suspect": suspect, "never_learned": self.never_learned.copy(),
                "forgotten": self.forgetting >= 1, "nonfinite": self.nonfinite > 0}

    def suspects(self, k=None, min_seen=2) -> np.ndarray:
        """The suspect entries, most negative mean margin first (ties by index); the first `k`."""
        idx = np.flatnonzero(self.flags(min_seen)["suspect"])
        idx = idx[np.lexsort((idx, self.mean_margin[idx]))]
        return idx if k is None else idx[:int(k)]

    def ambiguous(self, k) -> np.ndarray:
        """The `k` entries whose margin varied most over their finite visits (std_margin descending, ties by index)."""
        idx = np.flatnonzero(self.seen_finite > 0)
        idx = idx[np.lexsort((idx, -self.std_margin[idx]))]
        return idx[:int(k)]

    def misclassified(self) -> np.ndarray:
        """Entries with a wrong visit (correct < seen): after one evaluation pass, the clips the model gets wrong."""
        return np.flatnonzero(self.correct < self.seen)

    def keep(self, drop=("suspect",), **policy) -> np.ndarray:
        """A boolean mask over entries: False where a flag named in `drop` is set -- what `bank.loader(entries=...)` takes."""
        drop = (drop,) if isinstance(drop, str) else tuple(drop)
        unknown = [k for k in drop if k not in FLAG_NAMES]
        if unknown:
            raise ValueError(f"keep: unknown flag(s) {unknown}; expected names from {FLAG_NAMES}")
        f = self.flags(**policy)
        out = np.ones(len(self), bool)
        for k in drop:
            out &= ~f[k]
        return out

    def report(self, worst=5, **policy) -> str:
        """Plain text: the ledger in one line, the header's counters, counts per flag and per flag its `worst` entries."""
        f = self.flags(**policy)
        h, n = self.header, len(self)
        lines = [f"clip ledger: {n} entries, {h['rows']} rows in {h['updates']} updates, "
                 f"{bin(int(np.bitwise_or.reduce(self.seen_epochs)) if n else 0).count('1')} epochs recorded",
                 f"rows skipped: {h['skipped']}, entries out of range: {h['bad_entries']}, bad labels: {h['bad_labels']}, "
                 f"non-finite margins: {h['nonfinite']}",
                 f"flagged: {int(np.logical_or.reduce([f[k] for k in FLAG_NAMES]).sum()) if n else 0} of {n}"]
        mean = np.where(np.isnan(self.mean_margin), np.inf, self.mean_margin)
        severity = {"unseen": np.zeros(n), "suspect": -mean, "never_learned": -mean, "forgotten": self.forgetting.astype(np.float64),
                    "nonfinite": self.nonfinite.astype(np.float64)}
        for k in FLAG_NAMES:
            idx = np.flatnonzero(f[k])
            lines.append(f"  {k:<13} {idx.size:>7}")
            idx = idx[np.argsort(-severity[k][idx], kind="stable")][:worst]
            for e in idx:
                lines.append(f"      entry {int(e)}: seen {int(self.seen[e])}, correct {int(self.correct[e])}, mean margin {self.mean_margin[e]:+.4f}, "
                             f"std {self.std_margin[e]:.4f}, min {self.min_margin[e]:+.4f}, max {self.max_margin[e]:+.4f}, "
                             f"learned in epoch {int(self.learned_epoch[e])}, forgotten {int(self.forgetting[e])}x, "
                             f"non-finite {int(self.nonfinite[e])}")
        return "\n".join(lines)

    def __add__(self, other):
        """The report of a ledger that saw both row sets: sums added, bitmaps or-ed, min and max taken, headers added."""
        if not isinstance(other, LedgerReport):
            return NotImplemented
        if len(other) != len(self):
            raise ValueError(f"cannot add ledgers of {len(self)} and {len(other)} entries")
        a, b = self.entries, other.entries
        out = np.zeros(len(self), ENTRY_DTYPE)
        for k in ("sum_q", "sum_q2", "seen", "correct", "nonfinite"):
            out[k] = a[k] + b[k]
        for k in ("seen_epochs", "wrong_epochs"):
            out[k] = a[k] | b[k]
        out["min_q"], out["max_q"] = np.minimum(a["min_q"], b["min_q"]), np.maximum(a["max_q"], b["max_q"])
        header = {k: self.header[k] + other.header[k] for k in HEADER_FIELDS}
        return LedgerReport(header, out)


class ClipLedger:
    """`ClipLedger(n_entries, device)` or `ClipLedger.for_bank(bank)`: a cleared ledger on the device.

      begin_epoch()                    the next epoch: the first call makes `epoch` 0.  Past epoch 63 the bitmaps are full: `epoch` becomes
                                       -1 (one warning), the sums keep growing and the bitmaps stop.
      update(entries, logits, labels)  one launch: logits [B, 2] float32 and labels [B] or [B, 1] int64 on the device; `entries` [B] an
                                       int64 device tensor, or a host integer array (a loader's `last_entries`), uploaded once through
                                       pinned memory without a wait.  Rows with a negative entry are skipped.
      reset()                          clear the records and start again before epoch 0
      read() -> LedgerReport           the one device-to-host copy

    Before the first begin_epoch, `epoch` is -1: rows count everywhere but in the epoch bitmaps (an evaluation pass)."""

    SLOTS = 4                                                      # pinned staging buffers for host `entries`, used in turn

    def __init__(self, n_entries, device):
        from . import ops
        self.state = ops.new_clip_ledger(device, n_entries)
        self.n_entries = self.state.n_entries
        self.device = self.state.device
        self._begun = 0
        self._warned = False
        self._dev_entries = None
        self._pinned = None
        self._events = [None] * self.SLOTS
        self._used = [False] * self.SLOTS
        self._slot = 0

    @classmethod
    def for_bank(cls, bank):
        """A ledger with one record per entry of `bank`, on the bank's device."""
        if bank.device is None:
            raise ValueError("ClipLedger.for_bank: the bank holds nothing yet (no device)")
        return cls(bank.n_entries, bank.device)

    @property
    def epoch(self) -> int:
        return self._begun - 1 if 1 <= self._begun <= MAX_EPOCHS else -1

    def begin_epoch(self) -> int:
        self._begun += 1
        if self._begun > MAX_EPOCHS and not self._warned:
            self._warned = True
            warnings.warn(f"ClipLedger: epoch {self._begun - 1} lies past the {MAX_EPOCHS} epochs the bitmaps hold; the sums keep growing, "
                          "learned_epoch and forgetting stop at epoch 63", RuntimeWarning, stacklevel=2)
        return self.epoch

    def _upload(self, entries, B):
        """Host integers -> the persistent device buffer, through the next of SLOTS pinned rows: no wait unless the row's previous copy
        (SLOTS updates ago) is still in flight, and no allocation after the first call at a batch size."""
        import torch
        host = np.asarray(entries)
        if host.ndim != 1 or host.size != B or (B and host.dtype.kind not in "iu"):
            raise ValueError(f"entries: expected {B} integers, got {host.dtype} {host.shape}")
        with torch.cuda.device(self.device):
            if self._dev_entries is None or self._dev_entries.numel() < B:
                for ev in self._events:                            # the rows about to be replaced may still be read by a copy
                    if ev is not None:
                        ev.synchronize()
                self._dev_entries = torch.empty(B, device=self.device, dtype=torch.int64)
                self._pinned = torch.empty((self.SLOTS, B), dtype=torch.int64, pin_memory=True)
                self._events = [torch.cuda.Event() for _ in range(self.SLOTS)]
                self._used = [False] * self.SLOTS
            s = self._slot
            self._slot = (s + 1) % self.SLOTS
            if self._used[s] and not self._events[s].query():
                self._events[s].synchronize()
            row = self._pinned[s, :B]
            row.numpy()[:] = host
            dst = self._dev_entries[:B]
            dst.copy_(row, non_blocking=True)
            self._events[s].record()
            self._used[s] = True
        return dst

    def update(self, entries, logits, labels) -> None:
        import torch

        from . import ops
        labels = ops._check_ce(logits, labels)
        if not isinstance(entries, torch.Tensor):
            entries = self._upload(entries, logits.shape[0])
        ops.clip_ledger_update(logits, labels, entries, self.state, self.epoch)

    def reset(self) -> None:
        from . import ops
        ops.clip_ledger_reset(self.state)
        self._begun = 0
        self._warned = False

    def read(self) -> LedgerReport:
        from . import ops
        return ops.read_clip_ledger(self.state)
