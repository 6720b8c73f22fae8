"""ClipBank on the MI355X: the gather and peak kernels against their definitions in numpy float32 (bits; a
NaN must sit where the definition puts one -- the sign and payload of the NaN an invalid operation produces are the processor's
choice, x86 and gfx950 differ there, so NaNs are compared by position), banks past 2^31 samples, the bank loader against the file loader
batch for batch, stream entries, banks made from a Scan, and two epochs of training from either loader."""
import os
import random

import numpy as np
import pytest
import torch

import flacenc
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import bank as bankmod
from wakeword_jupyterlab_amd import scan
from wakeword_jupyterlab_amd.background import BackgroundNoiseBank
from wakeword_jupyterlab_amd.config import AudioConfig

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-3
DEV = torch.device("cuda", 0)


def _cfg(n):
    return type(f"AudioConfig{n}", (AudioConfig,), {"DURATION": n / 16000.0})


def _proc(n):
    return pkg.AudioProcessor(_cfg(n), device=DEV)


def _same_bits(got, want):
    """Equal float32 arrays as bits, NaNs by position."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn])


def _ref_row(x, start, n, norm, peak):
    """The definition: x the entry's samples (float32), numpy float32 division, np.fmax.reduce(|.|, initial=0)."""
    out = np.zeros(n, np.float32)
    j = np.arange(n)
    inside = (start + j >= 0) & (start + j < x.size)
    v = x[start + j[inside]]
    with np.errstate(invalid="ignore", divide="ignore"):
        if norm is None:
            out[inside] = v
        elif norm == "entry":
            out[inside] = v / np.float32(peak)
        else:
            p = np.fmax.reduce(np.abs(v), initial=np.float32(0))
            if p != 0:
                out[inside] = v / np.float32(p)
    return out


def _lengths(n):
    return [0, 1, 3, n - 1, n, n + 1, 3 * n + 7]


def _two_segments(n, seed):
    """A bank of two segments, each with entries of the lengths above back to back (odd lengths: every source alignment occurs)."""
    rng = np.random.default_rng(seed)
    b = pkg.ClipBank(_proc(n))
    xs = []
    for s in range(2):
        L = _lengths(n)
        x = (rng.standard_normal(sum(L)) * 0.3).astype(np.float32)
        b.add_buffer(torch.from_numpy(x).to(DEV), L, label=s)
        at = np.concatenate([[0], np.cumsum(L)])
        xs += [x[at[i]:at[i + 1]] for i in range(len(L))]
    return b, xs


_CASES = {}


def _gather_cases(n):
    """(bank, entries' samples, every (entry, start) pair of the issue's list) -- built once per N."""
    if n not in _CASES:
        b, xs = _two_segments(n, seed=n)
        pairs = []
        for e, x in enumerate(xs):
            L = x.size
            for s in sorted({0, 1, 2, 3, L - n, -5, -n, L - 1, L}):
                if -n <= s <= L:
                    pairs.append((e, s))
        random.Random(n).shuffle(pairs)
        _CASES[n] = (b, xs, pairs)
    return _CASES[n]


@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("n", [4000, 5001, 16000, 32000])
def test_gather_equals_the_definition(n, B):
    b, xs, pairs = _gather_cases(n)
    assert np.array_equal(b.peaks, np.array([np.fmax.reduce(np.abs(x), initial=np.float32(0)) for x in xs], np.float32))
    kinds = [None, "entry", "window"]
    if B == 1:
        pairs = pairs[::3]                                           # one row per launch: a third of the pairs, all three norms
    for rot in range(3):
        for c in range(0, len(pairs), B):
            chunk = pairs[c:c + B]
            norms = [kinds[(i + rot + c) % 3] for i in range(len(chunk))]      # the norms mix inside a batch
            got = b.gather([e for e, _ in chunk], [s for _, s in chunk], normalize=norms)
            assert got.shape == (len(chunk), n) and got.dtype == torch.float32 and got.device == DEV
            got = got.cpu().numpy()
            for r, ((e, s), k) in enumerate(zip(chunk, norms)):
                assert _same_bits(got[r], _ref_row(xs[e], s, n, k, b.peaks[e])), (n, e, s, k)


@pytest.mark.parametrize("n", [4000, 5001])
def test_gather_into_a_strided_out_leaves_the_rest_alone(n):
    b, xs, _ = _gather_cases(n)
    sentinel = -12345.5
    for pad in (3, 4):                                               # rows at every alignment, and rows 16-byte aligned
        out = torch.full((9, n + pad), sentinel, device=DEV)
        entries, starts, rows = [6, 13, 6, 3, 0], [5, n + 2, 5, -5, 0], [7, 0, 2, 5, 3]      # entry 6 twice in one batch
        back = b.gather(entries, starts, normalize="entry", out=out, rows=rows)
        assert back.data_ptr() == out.data_ptr()
        got = out.cpu().numpy()
        for e, s, r in zip(entries, starts, rows):
            assert _same_bits(got[r, :n], _ref_row(xs[e], s, n, "entry", b.peaks[e]))
        assert (got[:, n:] == sentinel).all() and (got[[1, 4, 6, 8]] == sentinel).all()
        assert np.array_equal(got[7, :n].view(np.uint32), got[2, :n].view(np.uint32))
    # a view whose row stride is larger than its width
    wide = torch.full((4, 2 * n), sentinel, device=DEV)
    b.gather([4, 5], [0, 1], normalize=None, out=wide[:, :n + 1], rows=[3, 1])
    got = wide.cpu().numpy()
    assert _same_bits(got[3, :n], _ref_row(xs[4], 0, n, None, 0)) and _same_bits(got[1, :n], _ref_row(xs[5], 1, n, None, 0))
    assert (got[:, n:] == sentinel).all() and (got[[0, 2]] == sentinel).all()


def test_gather_special_values():
    n = 4000
    rng = np.random.default_rng(9)
    x = (rng.standard_normal(3 * n + 7) * 0.3).astype(np.float32)
    x[100:100 + n + 50] = 0.0                                        # a silent stretch
    x[5000] = np.nan
    x[5001] = -0.0
    x[9000] = np.inf
    z = np.zeros(n - 1, np.float32)                                  # an all-zero entry: peak 0
    b = pkg.ClipBank(_proc(n))
    b.add_buffer(torch.from_numpy(np.concatenate([x, z])).to(DEV), [x.size, z.size])
    assert b.peaks[0] == np.inf and b.peaks[1] == 0.0
    # ENTRY with peak 0: NaN on the in-entry samples, +0 on the pad
    got = b.gather([1, 1], [0, -7], normalize="entry").cpu().numpy()
    assert np.isnan(got[0, :n - 1]).all() and got[0, n - 1:].view(np.uint32).tolist() == [0]
    assert (got[1, :7].view(np.uint32) == 0).all() and np.isnan(got[1, 7:]).all()
    # WINDOW on an all-zero window: zeros, never NaN -- inside the silent stretch and on the all-zero entry
    got = b.gather([0, 1, 0], [120, 0, 100], normalize="window").cpu().numpy()
    assert (got.view(np.uint32) == 0).all()
    # WINDOW with a NaN and a -0.0 in the window: the NaN is ignored by the peak and stays a NaN, -0.0 / p = -0.0
    got = b.gather([0, 0], [4500, 4999], normalize="window").cpu().numpy()
    for r, s in enumerate((4500, 4999)):
        want = _ref_row(x, s, n, "window", 0)
        assert _same_bits(got[r], want) and np.isnan(got[r, 5000 - s]) and np.isnan(got[r]).sum() == 1
        assert got[r, 5001 - s].view(np.uint32) == 0x80000000
        assert np.nanmax(np.abs(got[r])) == 1.0
    # an Inf in the window: p = Inf, finite samples become 0, Inf / Inf is NaN (numpy agrees)
    got = b.gather([0], [8000], normalize="window").cpu().numpy()
    assert _same_bits(got[0], _ref_row(x, 8000, n, "window", 0)) and np.isnan(got[0, 1000])


def _grid_items(n_items, g, pairs, silent):
    """(entry, start, norm) of item i = q g + r: pair i % len(pairs) and norm (r + q ((r // 3) % 3)) % 3 of (None, entry, window), so that
    over r the norms of item c and item c + g -- consecutive rows of one workgroup of a grid of g -- run through all nine ordered pairs.
    Asserted here: that, and that a silent window normalised by its own peak (the zero row) and an ordinary such window follow each
    other in a workgroup in both orders (red[] holds the peak of the window before)."""
    kinds = [None, "entry", "window"]
    items = [pairs[i % len(pairs)] + (kinds[(i % g + (i // g) * ((i % g // 3) % 3)) % 3],) for i in range(n_items)]
    assert n_items > 2 * g
    seen = {(items[c][2], items[c + g][2]) for c in range(n_items - g)}
    assert len(seen) == 9, seen
    quiet = [k == "window" and (e, s) in silent for e, s, k in items]
    loud = [k == "window" and (e, s) not in silent for e, s, k in items]
    assert any(quiet[c] and loud[c + g] for c in range(n_items - g)) and any(loud[c] and quiet[c + g] for c in range(n_items - g))
    return items


def test_gather_beyond_the_resident_grid():
    """bank_gather_kernel's grid is capped at 8 workgroups per CU and the other gather tests pass at most 37 items, so its loop over
    the items is never entered a second time.  Here 2 x 8 x CUs + 77 items at N = 4000 in ONE launch: every workgroup takes two rows
    and 77 take three.  WINDOW rows reduce their peak through red[] behind two barriers, the other norms meet no barrier, and
    _grid_items mixes the three norms between consecutive rows of a workgroup; among the windows are silent ones (the zero row), windows
    hanging over the front and over the end of their entry, entries shorter than a window and the empty entry.  Against the numpy
    definition of test_gather_equals_the_definition, bit for bit."""
    n = 4000
    g = 8 * torch.cuda.get_device_properties(DEV).multi_processor_count      # launch_bank_gather's cap
    n_items = 2 * g + 77
    rng = np.random.default_rng(77)
    L = [3 * n + 7, n - 1, 0, n + 1, 5, 2 * n]
    x = (rng.standard_normal(sum(L)) * 0.3).astype(np.float32)
    x[100:100 + n + 50] = 0.0                                            # a silent stretch in entry 0
    at = np.concatenate([[0], np.cumsum(L)])
    x[at[1]:at[2]] = 0.0                                                 # entry 1 is all zero: peak 0
    b = pkg.ClipBank(_proc(n))
    b.add_buffer(torch.from_numpy(x).to(DEV), L)
    xs = [x[at[i]:at[i + 1]] for i in range(len(L))]
    silent = {(0, 120), (0, 100), (1, 0), (1, -7), (2, 0)}
    pairs = sorted(silent) + [(0, 0), (0, -5), (0, -n), (0, L[0] - n), (0, L[0] - 3), (0, L[0]), (0, 2 * n + 1), (3, 1), (3, -n + 1), (3, 2),
                              (4, -17), (4, 5), (4, 0), (5, n), (5, n + 3), (5, -1), (5, n - 2), (0, 4101)]
    assert len(pairs) == 23 and all(-n <= s <= xs[e].size for e, s in pairs)          # a prime: no period shared with the norms or the grid
    items = _grid_items(n_items, g, pairs, silent)                                   # asserted before the launch
    got = b.gather([e for e, _, _ in items], [s for _, s, _ in items], normalize=[k for _, _, k in items])
    assert got.shape == (n_items, n) and got.dtype == torch.float32
    got = got.cpu().numpy()
    want = {}
    for r, (e, s, k) in enumerate(items):
        if (e, s, k) not in want:
            want[e, s, k] = _ref_row(xs[e], s, n, k, b.peaks[e])
        assert _same_bits(got[r], want[e, s, k]), (r, e, s, k)
    assert len(want) == 3 * len(pairs)
    zero_rows = [r for r, (e, s, k) in enumerate(items) if k == "window" and (e, s) in silent]
    assert len(zero_rows) > 100 and (got[zero_rows].view(np.uint32) == 0).all()


# ---- peaks ----------------------------------------------------------------------------------------------------------------------
def _np_peaks(x, lengths):
    at = np.concatenate([[0], np.cumsum(lengths)])
    return np.array([np.fmax.reduce(np.abs(x[at[i]:at[i + 1]]), initial=np.float32(0)) for i in range(len(lengths))], np.float32)


@pytest.mark.parametrize("shift", [0, 1, 3])
def test_peaks_equal_numpy(shift):
    rng = np.random.default_rng(4)
    L = [0, 1, 63, 64, 65, 100001, 0, 2 ** 20 + 3, 0]
    x = (rng.standard_normal(sum(L) + 11) * 0.5).astype(np.float32)       # 11 samples behind the last entry belong to nobody
    at = np.concatenate([[0], np.cumsum(L)])
    x[at[2]:at[3]] = -0.0                                                # an entry of all -0.0
    x[at[5]] = -7.0                                                      # the maximum at an entry's first sample,
    x[at[8] - 1] = 9.0                                                   # at another's last,
    x[at[5] + 4097] = np.nan                                             # NaNs inside are ignored,
    x[at[4]] = np.nan
    x[-3] = 100.0                                                        # and what lies behind offsets[n] is not looked at
    buf = torch.zeros(x.size + shift, device=DEV)
    buf[shift:] = torch.from_numpy(x).to(DEV)
    got = bankmod.bank_peaks(buf[shift:], at).cpu().numpy()              # a buffer at every 4-byte alignment
    want = _np_peaks(x, L)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[0] == 0 and got[2].view(np.uint32) == 0 and got[5] == 7.0 and got[7] == 9.0
    x[at[5] + 5] = np.inf
    buf[shift:] = torch.from_numpy(x).to(DEV)
    assert bankmod.bank_peaks(buf[shift:], at).cpu().numpy()[5] == np.inf


def test_peaks_of_one_entry_and_of_five_thousand():
    rng = np.random.default_rng(6)
    n = 1_000_003
    x = (rng.standard_normal(n) * 0.5).astype(np.float32)
    cuts = np.sort(rng.integers(0, n + 1, size=4999))                    # 5,000 entries of every length, empty ones included
    cuts[100:140] = cuts[100]                                            # forty empty entries in a row
    cuts[2000:3200] = np.sort(rng.integers(500_000, 500_900, size=1200)) # more entries inside one chunk than its table holds
    cuts = np.sort(cuts)
    at = np.concatenate([[0], cuts, [n]])
    data = torch.from_numpy(x).to(DEV)
    one = bankmod.bank_peaks(data, [0, n]).cpu().numpy()
    many = bankmod.bank_peaks(data, at).cpu().numpy()
    assert many.shape == (5000,) and np.array_equal(many.view(np.uint32), _np_peaks(x, np.diff(at)).view(np.uint32))
    assert one[0] == many.max() == np.abs(x).max()
    again = bankmod.bank_peaks(data, at).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), many.view(np.uint32))


def test_bank_past_two_to_the_31_samples():
    """An entry that starts past 2^31 samples, gathered at two starts (8.6 GB, freed after the test)."""
    n = 16000
    total = 2 ** 31 + 2 * n + 5
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < 4 * total + (2 << 30):
        pytest.fail(f"a bank of {total} samples needs {4 * total / 2**30:.1f} GiB; {free / 2**30:.1f} GiB free")
    data = torch.zeros(total, dtype=torch.float32, device=DEV)
    b = None
    try:
        ramp = (np.arange(2 * n, dtype=np.float32) - 700.0) / 8.0
        data[total - 2 * n:] = torch.from_numpy(ramp).to(DEV)           # a slice assignment: no full-size host array
        b = pkg.ClipBank(_proc(n))
        b.add_buffer(data, [2 ** 31 + 5, 2 * n])
        assert b._off[1] == 2 ** 31 + 5 and b.peaks[0] == 0.0 and b.peaks[1] == np.abs(ramp).max()
        got = b.gather([1, 1, 1], [0, n - 3, -2], normalize=[None, "entry", "window"]).cpu().numpy()
        assert _same_bits(got[0], _ref_row(ramp, 0, n, None, 0))
        assert _same_bits(got[1], _ref_row(ramp, n - 3, n, "entry", b.peaks[1]))
        assert _same_bits(got[2], _ref_row(ramp, -2, n, "window", 0))
    finally:
        del data
        b = None
        torch.cuda.empty_cache()


# ---- the loader is the file loader -------------------------------------------------------------------------------------------------
def _write(d, name, data):
    p = os.path.join(str(d), name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def _ints(n, seed):
    per = -(-n // 16000)
    x = np.concatenate([pkg.synth.make_clip(seed + j) for j in range(per)] + [np.zeros(0, np.float32)])[:n]
    return np.clip(np.round(x * 32767 * 0.8), -32768, 32767).astype(np.int64)


def _fourteen_files(d, n):
    w = lambda name, ints, rate=16000: _write(d, name, flacenc.wav_bytes(ints, rate, 16))   # noqa: E731
    wake = [w("w0.wav", _ints(6400, 1)),                                       # 0.4 s
            w("w1.wav", _ints(n, 2)),                                          # exactly N
            w("w2.wav", _ints(27200, 3)),                                      # 1.7 s
            w("w3.wav", flacenc.signal(57330, 2, 16, seed=4), 44100),          # 44.1 kHz stereo, 1.3 s
            w("w4.wav", _ints(7200, 5), 8000),                                 # 8 kHz, 0.9 s
            _write(d, "w5.flac", flacenc.encode(_ints(19200, 6), 16000, 16)),  # FLAC, 1.2 s
            w("w6.wav", _ints(n + 1, 7))]
    neg = [w("n0.wav", np.zeros(8000, np.int64)),                              # all zero: 0 / 0
           w("n1.wav", np.zeros(0, np.int64)),                                 # no frames
           _write(d, "n2.wav", b"this is not audio"),
           w("n3.wav", _ints(n - 1, 8)),
           w("n4.wav", _ints(36800, 9)),                                       # 2.3 s
           w("n5.wav", _ints(11200, 10)),
           w("n6.wav", _ints(40000, 11))]
    return wake, neg


def _epochs(loader, seed, k=2):
    random.seed(seed)
    torch.manual_seed(seed)
    return [[(d.clone(), t.clone()) for d, t in loader] for _ in range(k)]


def _equal_batches(a, b):
    assert len(a) == len(b)
    for ea, eb in zip(a, b):
        assert len(ea) == len(eb) > 0
        for (da, ta), (db, tb) in zip(ea, eb):
            assert torch.equal(ta, tb) and da.shape == db.shape
            na, nb = torch.isnan(da), torch.isnan(db)
            assert torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(da), da), torch.where(nb, torch.zeros_like(db), db))


@pytest.mark.parametrize("duration, augment, background", [(1.0, False, False), (1.0, True, False), (0.5, False, False), (0.5, True, False),
                                                           (1.0, True, True)])
def test_bank_loader_is_the_file_loader(tmp_path, capsys, duration, augment, background):
    n = int(16000 * duration)
    wake, neg = _fourteen_files(tmp_path, n)
    proc = _proc(n)
    if background:
        noise = (np.random.default_rng(2).standard_normal(50000) * 0.1).astype(np.float32)
        proc.set_background_noise(BackgroundNoiseBank.from_buffer(torch.from_numpy(noise).to(DEV), [30000, 20000]))
    ds = pkg.WakewordDataset(wake, neg, proc, augment=augment, verbose=False)
    b = pkg.ClipBank.from_dataset(ds)
    assert b.n_entries == b.n_items == 14 and b.labels.tolist() == ds.labels and b.unreadable == 1 and not b.ok[9]
    for i, p in enumerate(ds.files):                                           # the stored samples are load_audio's, bit for bit
        if b.ok[i]:
            a = proc.load_audio(p)
            o = int(b._off[i])
            assert np.array_equal(b.segments[0][o:o + int(b.lengths[i])].cpu().numpy().view(np.uint32), a.view(np.uint32))
    want = _epochs(ds.loader(5, shuffle=True), seed=7)
    got = _epochs(b.loader(5, shuffle=True, augment=augment), seed=7)
    _equal_batches(got, want)
    assert ds.unreadable == 2 * b.unreadable                                   # the dataset counts a file once per epoch it is served
    assert any(torch.isnan(d).any() for d, _ in want[0])                       # the all-zero file is 0 / 0 in both
    got2 = _epochs(pkg.DataLoader(ds.cache(), batch_size=5, shuffle=True, augment=augment), seed=7, k=1)
    _equal_batches(got2, want[:1])
    capsys.readouterr()


def test_stream_entries(tmp_path):
    n = 16000
    ints = _ints(160000, 21)
    ints[30000:30000 + 2 * n + 100] = 0                                        # a silent stretch longer than a window
    long_p = _write(tmp_path, "long.wav", flacenc.wav_bytes(ints, 16000, 16))
    short_p = _write(tmp_path, "short.wav", flacenc.wav_bytes(_ints(5000, 22), 16000, 16))
    proc = _proc(n)
    b = pkg.ClipBank(proc)
    b.add_recordings([long_p, short_p], label=0, windows_per_epoch=7)
    assert b.n_entries == 2 and b.n_items == 14 and b.item_entries().tolist() == [0] * 7 + [1] * 7
    x = [proc.load_audio(long_p), proc.load_audio(short_p)]
    seen = []
    inner = b._gather
    b._gather = lambda *a, **k: seen.append(inner(*a, **k)) or seen[-1]
    random.seed(3)
    batches = list(b.loader(4))
    rows = torch.cat(seen).cpu().numpy()
    random.seed(3)
    for r in range(14):
        e = 0 if r < 7 else 1
        s = random.randint(0, x[e].size - n) if x[e].size > n else 0          # the short recording: start 0, zero pad, no draw
        assert _same_bits(rows[r], _ref_row(x[e], s, n, "window", 0)), r
    assert np.abs(rows).max() == 1.0 and (rows[7:, 5000:] == 0).all()
    assert sum(d.shape[0] for d, _ in batches) == 14 and all(torch.isfinite(d).all() for d, _ in batches)
    assert all((t == 0).all() and t.shape == (d.shape[0], 1) for d, t in batches)
    # a window over the silent stretch: zeros (not 0 / 0), and a finite mel batch
    quiet = b.gather([0, 0], [30050, 70000], normalize="window")
    assert (quiet[0] == 0).all() and quiet[1].abs().max() == 1.0
    assert torch.isfinite(proc.mel_batch(quiet, normalize=False)).all()
    # the default: ceil(len / N) windows
    b2 = pkg.ClipBank(proc)
    b2.add_recordings([long_p, short_p])
    assert b2.windows.tolist() == [10, 1] and b2.n_items == 11


def _model(n, seed=1234):
    sd = pkg.synth.make_state_dict("simple", seed=seed)
    m = pkg.SimpleWakewordModel(audio_config=_cfg(n))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV).eval()


def test_bank_from_a_scan(tmp_path):
    n = 8000
    m = _model(n)
    neg = [_write(tmp_path, f"n{i}.wav", flacenc.wav_bytes(_ints(40000 + 777 * i, 200 + 3 * i), 16000, 16)) for i in range(3)]
    s = scan.scan_files(m, neg, hop_samples=160)
    proc = _proc(n)
    b = pkg.ClipBank(proc)
    b.add_recordings(s)
    assert b.segments[0].data_ptr() == s.audio.data_ptr() and b.lengths.tolist() == s.lengths.tolist()      # shared, not copied
    assert b.kinds.tolist() == [bankmod.STREAM] * 3 and b.windows.tolist() == [-(-int(L) // n) for L in s.lengths]
    for i in range(3):
        a = s.audio[int(s.offsets[i]):int(s.offsets[i] + s.lengths[i])].cpu().numpy()
        assert b.peaks[i] == np.abs(a).max()
    prob = s.prob.cpu().numpy()
    theta = float(np.sort(prob)[-12])                                          # a threshold that a handful of windows pass
    pcm, files, times = s.hard_negatives(theta, refractory_s=0.0)
    M = pcm.shape[0]
    assert M >= 2
    mined = b.add_pcm(pcm, 0)
    assert list(mined) == list(range(3, 3 + M)) and b.n_items == int(b.windows[:3].sum()) + M
    back = b.gather(list(mined), normalize=None)
    assert torch.equal(back, pcm)                                              # trained on exactly as the detector saw it
    with torch.no_grad():
        logits = m.forward_pcm(b.gather(list(mined), normalize="entry"), normalize=False)
    p = (1.0 / (1.0 + torch.exp(logits[:, 0] - logits[:, 1]))).cpu().numpy()
    k = np.round(times * 16000 / 160).astype(np.int64)                         # the 1-based window numbers
    at = s.window_offsets[files] + k - 1
    assert np.abs(p - prob[at]).max() <= LOGIT_TOL


def test_training_from_the_bank_equals_training_from_files(tmp_path, capsys):
    n = 16000
    files = [_write(tmp_path, f"f{i:02d}.wav", flacenc.wav_bytes(_ints(9000 + 1500 * i, 40 + i), 16000, 16)) for i in range(24)]
    proc = _proc(n)
    ds = pkg.WakewordDataset(files[:12], files[12:], proc, augment=True, verbose=False)

    def train(loader):
        random.seed(5)
        torch.manual_seed(5)
        model = pkg.SimpleWakewordModel().to(DEV).train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        crit = torch.nn.CrossEntropyLoss()
        losses = []
        for _ in range(2):
            for data, target in loader:
                opt.zero_grad()
                loss = crit(model(data), target.squeeze(1))
                loss.backward()
                opt.step()
                losses.append(loss.item())
        return losses
    want = train(ds.loader(8, shuffle=True))
    got = train(ds.cache().loader(8, shuffle=True, augment=True))
    assert len(want) == 6 and np.isfinite(want).all() and got == want
    capsys.readouterr()
