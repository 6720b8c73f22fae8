"""The clip ledger on the MI355X: the device buffer against the sequential restatement (tests/ledger_ref.py)
byte for byte, header included; order and split independence; guard bands; the trainer, the loaders and evaluate_report with a ledger;
and planted label errors found by their negative mean margin.

Out-of-range entries used on the device are -1, -2, n_entries, n_entries + 3 and 2^32 + 1 only: a kernel that checked nothing would put
the first four inside this file's own guard bands, and one that truncated the last to 32 bits would write entry 1 (inside the ledger, or
the back guard when n_entries is 1).  Nothing larger is fed."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import ledger_ref as ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import ops
from wakeword_jupyterlab_amd.ledger import ClipLedger, LedgerReport

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
L = nat.lib
GUARD = 4096
POISON = 0xA5
EPOCHS = (0, 31, 32, 63, -1)                                       # the boundaries of the 64-bit shifts, and "no epoch bit"


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Guarded:
    """A ledger between two 4 KiB guard bands, everything poisoned."""

    def __init__(self, n_entries, fill=POISON):
        self.n_entries = n_entries
        self.nbytes = nat.check(L.ww_clip_ledger_bytes(n_entries))
        assert self.nbytes == 64 + 56 * n_entries
        self.raw = torch.full((2 * GUARD + self.nbytes,), fill, dtype=torch.uint8, device=DEV)
        self.raw[:GUARD] = POISON
        self.raw[GUARD + self.nbytes:] = POISON
        self.ptr = self.raw.data_ptr() + GUARD
        assert self.ptr % 8 == 0

    def init(self):
        nat.check(L.ww_clip_ledger_init(self.ptr, self.n_entries, _stream()))

    def update(self, z, y, e, epoch):
        nat.check(L.ww_clip_ledger_update_f32(z.data_ptr(), y.data_ptr(), e.data_ptr(), z.shape[0], epoch, self.ptr, self.n_entries, _stream()))

    def bytes(self):
        host = self.raw.cpu().numpy()
        assert (host[:GUARD] == POISON).all() and (host[GUARD + self.nbytes:] == POISON).all(), "a guard band was written"
        return host[GUARD:GUARD + self.nbytes].tobytes()


def _inputs(n, n_entries, seed):
    """n rows with every special case of the contract that fits into n rows, at scattered positions."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((n, 2)) * 3).astype(np.float32)
    y = rng.integers(0, 2, n).astype(np.int64)
    e = rng.integers(0, n_entries, n).astype(np.int64)
    pos = iter(rng.permutation(n).tolist())

    def put(z0=None, z1=None, label=None, entry=None):
        i = next(pos, None)
        if i is None:
            return
        if z0 is not None:
            z[i] = (z0, z1)
        if label is not None:
            y[i] = label
        if entry is not None:
            e[i] = entry
    for bad in (-1, -2, n_entries, n_entries + 3, 2 ** 32 + 1):
        put(entry=bad)
    for bad in (-100, 2):
        put(label=bad)
    put(1.25, 1.25), put(-0.0, 0.0), put(np.nan, 0.0), put(0.0, np.nan), put(np.inf, 0.0), put(0.0, np.inf), put(0.0, -np.inf)
    put(np.inf, np.inf), put(3e38, -3e38)                                   # inf - inf = NaN; an overflowing subtraction
    put(0.0, 100.0), put(0.0, -90.0), put(70.0, -1.0), put(0.0, 64.0), put(0.0, -64.0), put(0.0, np.nextafter(np.float32(64), np.float32(65)))
    for k in (0, 1, 2, 3, -1, -2, -3, 1000001, 4194302):                    # exact halves of 2^-16: round half to even
        put(0.0, (k + 0.5) / 65536.0)
    put(entry=-1, label=7), put(entry=n_entries, label=-100)                # the entry decides first: skipped / bad entry, not bad label
    return z, y, e


@pytest.mark.parametrize("n_entries", [1, 7, 300])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_ledger_is_the_restatement_byte_for_byte(n, n_entries):
    g = _Guarded(n_entries)
    g.init()
    want = ref.RefLedger(n_entries)
    assert g.bytes() == want.tobytes()                                      # cleared: min_q = INT32_MAX, max_q = INT32_MIN
    counts = dict(rows=0, skipped=0, bad_entries=0)
    for k, epoch in enumerate(EPOCHS):
        z, y, e = _inputs(n, n_entries, seed=1000 * n + 10 * n_entries + k)
        want.update(z, y, e, epoch)
        g.update(torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV), torch.from_numpy(e).to(DEV), epoch)
        counts["rows"] += n
        counts["skipped"] += int((e < 0).sum())
        counts["bad_entries"] += int((e >= n_entries).sum())
    got = g.bytes()                                                         # checks both guard bands
    rep = LedgerReport.from_buffer(got, n_entries)
    assert {k: rep.header[k] for k in counts} == counts and rep.header["updates"] == len(EPOCHS)
    if n >= 65:
        assert rep.header["skipped"] >= 5 and rep.header["bad_entries"] >= 5 and rep.header["bad_labels"] >= 5 and rep.header["nonfinite"] >= 5
    assert rep.header == {k: want.header[k] for k in ref.HEADER_FIELDS}
    for name in rep.entries.dtype.names:
        assert np.array_equal(rep.entries[name], LedgerReport.from_buffer(want.tobytes(), n_entries).entries[name]), name
    assert got == want.tobytes()
    if n == 1000 and n_entries == 1:                                        # every scored row on one record
        assert rep.seen[0] == sum(len(v) for v in want.visits) > 4800


def test_order_and_split_independence():
    """The same 1000 rows, permuted, as batches of 1, 64 and 1000: identical bytes, except the header's `updates`, which counts calls."""
    n, n_entries = 1000, 7
    z, y, e = _inputs(n, n_entries, seed=3)
    want = ref.RefLedger(n_entries)
    want.update(z, y, e, 5)
    results = []
    for split, seed in ((1000, None), (64, 1), (1, 2), (1000, 4)):
        order = np.arange(n) if seed is None else np.random.default_rng(seed).permutation(n)
        zt, yt, et = (torch.from_numpy(a[order]).to(DEV) for a in (z, y, e))
        state = ops.new_clip_ledger(DEV, n_entries)
        for s in range(0, n, split):
            ops.clip_ledger_update(zt[s:s + split], yt[s:s + split], et[s:s + split], state, epoch=5)
        rep = ops.read_clip_ledger(state)
        assert rep.header["updates"] == -(-n // split)
        rep.header["updates"] = 1
        results.append(rep.tobytes())
    assert results[0] == want.tobytes()
    assert results[1] == results[0] and results[2] == results[0] and results[3] == results[0]


def test_init_does_not_depend_on_the_buffer_and_reset_clears():
    n_entries = 300
    images = []
    for fill in (POISON, 0, 0xFF):
        g = _Guarded(n_entries, fill)
        g.init()
        images.append(g.bytes())
    assert images[0] == images[1] == images[2] == ref.RefLedger(n_entries).tobytes()
    empty = _Guarded(0)
    empty.init()
    assert empty.bytes() == ref.RefLedger(0).tobytes() and len(empty.bytes()) == 64
    z, y, e = _inputs(257, n_entries, seed=8)
    lg = ClipLedger(n_entries, DEV)
    assert lg.epoch == -1 and lg.read().tobytes() == images[0]
    assert lg.begin_epoch() == 0 and lg.begin_epoch() == 1
    lg.update(e, torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV).view(-1, 1))         # host entries, [n, 1] labels
    want = ref.RefLedger(n_entries)
    want.update(z, y, e, 1)
    assert lg.read().tobytes() == want.tobytes()
    lg.reset()
    assert lg.epoch == -1 and lg.read().tobytes() == images[0]
    # the wrappers' checks
    zt, yt, et = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV), torch.from_numpy(e).to(DEV)
    with pytest.raises(TypeError):
        ops.clip_ledger_update(zt, yt, et.int(), lg.state)
    with pytest.raises(ValueError):
        ops.clip_ledger_update(zt, yt, et[:5], lg.state)
    with pytest.raises(ValueError, match="epoch"):
        ops.clip_ledger_update(zt, yt, et, lg.state, epoch=64)
    with pytest.raises(RuntimeError):
        ops.clip_ledger_update(zt, yt, et.cpu(), lg.state)
    with pytest.raises(TypeError):
        ops.clip_ledger_update(zt, yt, et, ops.new_loss_stats(DEV))
    with pytest.raises(ValueError):
        lg.update(e[:9], zt, yt)
    with pytest.raises(ValueError):
        ops.new_clip_ledger(DEV, -1)
    with pytest.raises(RuntimeError):
        ops.new_clip_ledger("cpu", 4)
    assert lg.read().tobytes() == images[0]                                 # none of the refused calls wrote


# ---- trainer ----------------------------------------------------------------------------------------------------------------------
def _batch(n, T, seed):
    g = torch.Generator().manual_seed(seed)
    x = (-40.0 + 20.0 * torch.randn(n, 1, 80, T, generator=g)).to(DEV)
    y = torch.randint(0, 2, (n, 1), generator=g).to(DEV)
    return x, y


def _simple(seed=1234):
    torch.manual_seed(seed)
    return pkg.SimpleWakewordModel().to(DEV)


class _Named(list):
    """Batches with the attribute the ledger scatters by: a loader in miniature."""

    def __init__(self, batches, entries):
        super().__init__(batches)
        self._entries, self.last_entries = entries, None

    def __iter__(self):
        for b, e in zip(list.__iter__(self), self._entries):
            self.last_entries = e
            yield b


def test_trainer_with_a_ledger_trains_the_same_and_records_its_logits():
    B, T, n_entries = 37, 31, 50
    rng = np.random.default_rng(1)
    entries = [rng.integers(0, n_entries, B).astype(np.int64) for _ in range(3)]
    entries[0][:3] = 11                                                     # an entry three times in one batch
    entries[1][5] = -1                                                      # a placeholder row
    batches = [_batch(B, T, seed=30 + t) for t in range(3)]

    def run(ledger):
        model = _simple()
        trainer = pkg.WakewordTrainer(model, DEV, ledger=ledger)
        model.train()
        torch.manual_seed(77)
        logits = []
        for t, (x, y) in enumerate(batches):
            if ledger is not None and t != 1:
                ledger.begin_epoch()                                        # steps 0 and 1 in epoch 0, step 2 in epoch 1
            trainer.step(x, y, entries=entries[t])
            logits.append(trainer.last_logits[:B].cpu().numpy().copy())
        return model, trainer, logits
    lg = ClipLedger(n_entries, DEV)
    plain, _, plain_logits = run(None)
    model, trainer, logits = run(lg)
    for (k, p), (_, q) in zip(model.named_parameters(), plain.named_parameters()):
        assert torch.equal(p, q), k
    assert all(np.array_equal(a, b) for a, b in zip(logits, plain_logits))
    want = ref.RefLedger(n_entries)
    for t, epoch in enumerate((0, 0, 1)):
        want.update(logits[t], batches[t][1].cpu().numpy(), entries[t], epoch)
    rep = lg.read()
    assert rep.tobytes() == want.tobytes()
    assert rep.header["rows"] == 3 * B and rep.header["skipped"] == 1 and rep.seen[11] >= 3
    # after the warm-up a step with a ledger waits for nothing and allocates nothing
    x, y = batches[0]
    y = y.contiguous()
    for _ in range(2):
        trainer.step(x, y, entries=entries[0])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        trainer.step(x, y, entries=entries[0])
        trainer.step(x, y, entries=entries[2])
        before = torch.cuda.memory_allocated()
        for _ in range(ClipLedger.SLOTS + 1):                               # every staging row is used again
            trainer.step(x, y, entries=entries[1])
        after = torch.cuda.memory_allocated()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert before == after
    torch.cuda.synchronize()
    assert lg.read().header["updates"] == 3 + 2 + 2 + ClipLedger.SLOTS + 1


def test_train_epoch_and_validate_fill_their_ledgers():
    B, n_entries = 16, 20
    model = _simple()
    lg, vlg = ClipLedger(n_entries, DEV), ClipLedger(n_entries, DEV)
    trainer = pkg.WakewordTrainer(model, DEV)
    assert trainer.ledger is None and trainer.val_ledger is None
    trainer.ledger, trainer.val_ledger = lg, vlg                            # assignable
    x, y = _batch(37, 8, seed=8)
    batches = [(x[i:i + B], y[i:i + B]) for i in range(0, 37, B)]           # 16, 16 and a ragged 5
    entries = [np.arange(i, min(i + B, 37), dtype=np.int64) % n_entries for i in range(0, 37, B)]
    with pytest.raises(TypeError, match="last_entries"):
        trainer.train_epoch(batches)                                        # a plain list names no rows: refused at the first batch
    lg.reset()
    seen = []
    real = lg.update
    lg.update = lambda e, z, t: (seen.append(z.cpu().numpy().copy()), real(e, z, t))[1]
    torch.manual_seed(1)
    for _ in range(2):
        trainer.train_epoch(_Named(batches, entries))
    want = ref.RefLedger(n_entries)
    for k, z in enumerate(seen):
        want.update(z, batches[k % 3][1].cpu().numpy(), entries[k % 3], k // 3)
    assert len(seen) == 6 and lg.read().tobytes() == want.tobytes() and lg.epoch == 1
    trainer.validate(_Named(batches, entries))
    with torch.no_grad():
        outs = [model(xb).cpu().numpy() for xb, _ in batches]
    vwant = ref.RefLedger(n_entries)
    for z, (_, yb), e in zip(outs, batches, entries):
        vwant.update(z, yb.cpu().numpy(), e, 0)
    assert vlg.read().tobytes() == vwant.tobytes()
    with pytest.raises(TypeError, match="last_entries"):
        trainer.validate(batches)


# ---- loaders ----------------------------------------------------------------------------------------------------------------------
def _epochs(loader, seed, k=2):
    random.seed(seed)
    torch.manual_seed(seed)
    out = []
    for _ in range(k):
        out.append([(d.clone(), t.clone(), loader.last_entries.copy()) for d, t in loader])
    return out


def test_loaders_name_their_rows_and_entries_selects(tmp_path, capsys):
    proc = pkg.AudioProcessor(device=DEV)
    N = 16000
    # ---- the file loader: last_entries are indices into ds.files, -1 for the unreadable file ----
    wake, neg = [], []
    for i in range(9):
        p = str(tmp_path / f"c{i}.wav")
        pkg.synth.write_wav16(p, pkg.synth.make_clip(i) * 0.9)
        (wake if i % 3 == 0 else neg).append(p)
    broken = str(tmp_path / "broken.wav")
    with open(broken, "wb") as f:
        f.write(b"this is not audio")
    neg.insert(2, broken)
    ds = pkg.WakewordDataset(wake, neg, proc, verbose=False)
    bank = ds.cache()
    bad = ds.files.index(broken)
    for loader in (ds.loader(4, shuffle=True), bank.loader(4, shuffle=True)):
        assert loader.last_entries is None
        rows = []
        for data, target, le in _epochs(loader, seed=5, k=1)[0]:
            assert le.dtype == np.int64 and le.shape == (data.shape[0],)
            real = np.where(le < 0, bad, le)
            assert target[:, 0].tolist() == [ds.labels[i] for i in real]
            direct = proc.mel_batch(bank.gather(real), normalize=False)     # the clips are exactly N samples: every window starts at 0
            direct[torch.from_numpy(le < 0).to(DEV)] = 0.0
            assert torch.equal(data, direct)
            rows += le.tolist()
        assert sorted(rows) == sorted([-1] + [i for i in range(10) if i != bad])
    capsys.readouterr()
    # ---- entries=mask: the unmasked loader of a bank built from the subset, bit for bit (clips longer than N: the starts are drawn) ----
    pcm = np.concatenate([pkg.synth.make_clips(20, 13), pkg.synth.make_clips(40, 13)[:, :4000]], axis=1)
    labels = (np.arange(13) % 3 == 0).astype(np.int64)
    mask = np.array([1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 0, 1], bool)
    full, sub = pkg.ClipBank(proc), pkg.ClipBank(proc)
    full.add_pcm(pcm, labels)
    sub.add_pcm(pcm[mask], labels[mask])
    for kw in (dict(shuffle=True), dict(shuffle=False, drop_last=True), dict(shuffle=True, positive_fraction=0.5)):
        a = full.loader(3, entries=mask, **kw)
        b = sub.loader(3, **kw)
        assert len(a) == len(b) and len(a.order()) == len(b.order())
        got, want = _epochs(a, seed=9), _epochs(b, seed=9)
        for ea, eb in zip(got, want):
            assert len(ea) == len(eb) > 0
            for (da, ta, la), (db, tb, lb) in zip(ea, eb):
                assert torch.equal(da, db) and torch.equal(ta, tb)
                assert np.array_equal(la, np.flatnonzero(mask)[lb])         # last_entries stay in the full bank's coordinates
    by_index = [tuple(la) for ep in _epochs(full.loader(3, entries=np.flatnonzero(mask)), 9) for _, _, la in ep]
    assert by_index == [tuple(la) for ep in _epochs(full.loader(3, entries=mask), 9) for _, _, la in ep]
    # ---- entries=None is the loader it always was ----
    got, want = _epochs(full.loader(4, shuffle=True, entries=None), seed=2), _epochs(full.loader(4, shuffle=True), seed=2)
    assert all(torch.equal(da, db) and torch.equal(ta, tb) and np.array_equal(la, lb)
               for ea, eb in zip(got, want) for (da, ta, la), (db, tb, lb) in zip(ea, eb))
    assert ClipLedger.for_bank(full).n_entries == 13


# ---- what it is for ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noisy_bank():
    """96 synthetic 1 s clips, label i % 3 == 0, six labels flipped."""
    proc = pkg.AudioProcessor(device=DEV)
    labels = (np.arange(96) % 3 == 0).astype(np.int64)
    flipped = np.sort(np.random.RandomState(7).choice(96, 6, replace=False))
    labels[flipped] ^= 1
    bank = pkg.ClipBank(proc)
    bank.add_pcm(pkg.synth.make_clips(0, 96), labels)
    return bank, flipped


def test_planted_label_errors_are_the_suspects(noisy_bank):
    """30 epochs of batch 16, shuffled, Adam at 1e-3, no dropout: the six flipped clips are exactly the clips with a negative mean
    margin.  A condition, not a tolerance: the same arithmetic on the CPU leaves more than 1.5 logit units on either side of zero."""
    bank, flipped = noisy_bank
    torch.manual_seed(0)
    random.seed(0)
    model = pkg.SimpleWakewordModel().to(DEV)
    model.lstm.dropout = 0.0
    model.dropout.p = 0.0
    cfg = type("Cfg", (pkg.TrainingConfig,), {"LEARNING_RATE": 1e-3})
    ledger = ClipLedger.for_bank(bank)
    trainer = pkg.WakewordTrainer(model, DEV, cfg, ledger=ledger)
    loader = bank.loader(16, shuffle=True)
    for _ in range(30):
        trainer.train_epoch(loader)
    rep = ledger.read()
    clean = np.setdiff1d(np.arange(96), flipped)
    print(f"mean margin: flipped max {rep.mean_margin[flipped].max():+.3f}, clean min {rep.mean_margin[clean].min():+.3f}")
    print(rep.report(worst=6))
    assert rep.header["rows"] == 30 * 96 and rep.header["updates"] == 30 * 6 and (rep.seen == 30).all()
    assert (rep.seen_epochs == (1 << 30) - 1).all()
    assert set(rep.suspects().tolist()) == set(flipped.tolist())
    assert not rep.flags()["suspect"][clean].any() and rep.flags()["suspect"][flipped].all()
    # and the way out: the loader without them, or with their labels turned
    keep = rep.keep()
    assert keep.sum() == 90 and len(bank.loader(16, entries=keep)) == 6


def test_evaluate_report_fills_a_ledger(noisy_bank):
    bank, _ = noisy_bank
    sd = pkg.synth.make_state_dict("simple", seed=1234)
    model = pkg.SimpleWakewordModel()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(DEV).eval()
    ledger = ClipLedger.for_bank(bank)
    loader = bank.loader(40)
    report = pkg.evaluate_report(model, loader, ledger=ledger)
    with torch.no_grad():
        z = torch.cat([model(d) for d, _ in loader]).cpu().numpy()
    pred = (z[:, 1] > z[:, 0]).astype(np.int64)
    rep = ledger.read()
    assert (rep.seen == 1).all() and (rep.seen_epochs == 0).all() and rep.header["updates"] == 3
    assert rep.misclassified().tolist() == np.flatnonzero(pred != bank.labels).tolist()
    assert int(rep.correct.sum()) == int(report.confusion[0][0] + report.confusion[1][1])
    want = ref.RefLedger(96)
    want.update(z, bank.labels, np.arange(96), -1)
    want.header["updates"] = 3
    assert rep.tobytes() == want.tobytes()
    with pytest.raises(TypeError, match="last_entries"):
        pkg.evaluate_report(model, list(loader), ledger=ledger)
