"""ClipBank without a GPU: the argument checks of ww_bank_peaks_f32 / ww_bank_gather_f32 come before any
device call and name the field; the ctypes item is the header's struct; the loader's item list, order and `random` draws, run against a
stand-in gather; the package DataLoader routes a bank to bank.loader with the refusals it has for a dataset."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import bank as bankmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 16000


def _items(**kw):
    it = (nat.BankItem * 1)()
    it[0].offset, it[0].length, it[0].start, it[0].peak, it[0].row, it[0].norm = 0, 20000, 0, 1.0, 0, nat.BANK_NORM_ENTRY
    for k, v in kw.items():
        setattr(it[0], k, v)
    return it


def _gather(items, n_items=1, n=N, total=50000, n_rows=4, stride=None):
    # device pointers null: every check of a field comes first
    return nat.lib.ww_bank_gather_f32(None, total, items, n_items, n, None, n_rows, n if stride is None else stride, None, None)


@pytest.mark.parametrize("kw, call, word", [
    ({}, dict(n=3999), b"n_samples"),
    ({}, dict(n=32001), b"n_samples"),
    ({}, dict(stride=N - 1), b"out_stride"),
    ({"start": 20001}, {}, b"start"),
    ({"start": -N - 1}, {}, b"start"),
    ({"offset": 30001}, {}, b"total_samples"),
    ({"offset": -1}, {}, b"offset"),
    ({"length": -1}, {}, b"length"),
    ({"norm": 3}, {}, b"norm"),
    ({"peak": -0.5}, {}, b"peak"),
    ({"row": 4}, {}, b"row"),
    ({"row": -1}, {}, b"row"),
])
def test_gather_argument_checks_name_the_field(kw, call, word):
    assert _gather(_items(**kw), **call) == nat.WW_EINVAL
    assert word in nat.lib.ww_last_error()


def test_gather_refuses_a_row_named_twice_and_null_pointers():
    it = (nat.BankItem * 2)()
    for i in range(2):
        it[i].offset, it[i].length, it[i].start, it[i].peak, it[i].row, it[i].norm = 0, 100, 0, 1.0, 1, nat.BANK_NORM_NONE
    assert _gather(it, n_items=2) == nat.WW_EINVAL and b"twice" in nat.lib.ww_last_error()
    it[1].row = 2
    assert _gather(it, n_items=2) == nat.WW_EINVAL and b"null" in nat.lib.ww_last_error()      # the items pass; the pointers do not
    assert _gather(None, n_items=1) == nat.WW_EINVAL and b"items" in nat.lib.ww_last_error()
    assert _gather(None, n_items=0) == nat.WW_OK                                                # nothing to do
    # the bounds of start are inclusive: -N and length pass the item checks
    for s in (-N, 100):
        it[0].start = s
        assert _gather(it, n_items=2) == nat.WW_EINVAL and b"null" in nat.lib.ww_last_error()
    assert nat.lib.ww_bank_gather_workspace_bytes(-1) == nat.WW_EINVAL
    assert nat.lib.ww_bank_gather_workspace_bytes(3) == 256 and nat.lib.ww_bank_gather_workspace_bytes(4096) == 4096 * 40


def test_peaks_argument_checks():
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    assert nat.lib.ww_bank_peaks_f32(None, -1, None, 1, None, None) == nat.WW_EINVAL and b"total_samples" in nat.lib.ww_last_error()
    assert nat.lib.ww_bank_peaks_f32(None, 10, None, -1, None, None) == nat.WW_EINVAL and b"n_entries" in nat.lib.ww_last_error()
    assert nat.lib.ww_bank_peaks_f32(None, 10, None, 1, None, None) == nat.WW_EINVAL and b"null" in nat.lib.ww_last_error()
    assert nat.lib.ww_bank_peaks_f32(p + 2, 10, p, 1, p, None) == nat.WW_EINVAL and b"aligned" in nat.lib.ww_last_error()
    assert nat.lib.ww_bank_peaks_f32(p, 10, p + 4, 1, p, None) == nat.WW_EINVAL and b"aligned" in nat.lib.ww_last_error()
    assert nat.lib.ww_bank_peaks_f32(None, 10, None, 0, None, None) == nat.WW_OK
    if not torch.cuda.is_available():
        assert nat.lib.ww_bank_peaks_f32(p, 10, p, 1, p, None) == nat.WW_ENODEVICE


def test_item_struct_is_the_headers(tmp_path):
    text = open(os.path.join(ROOT, "include", "wakeword_amd.h")).read()
    body = re.search(r"typedef struct ww_bank_item \{(.*?)\} ww_bank_item;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int64_t|int32_t|float)\s+(\w+)\s*;", body)
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(nat.BankItem._fields_)
    size = {"int64_t": 8, "int32_t": 4, "float": 4}
    at = 0
    for t, n in fields:                                           # natural alignment, as the C ABI lays a struct out
        at = -(-at // size[t]) * size[t]
        assert getattr(nat.BankItem, n).offset == at
        at += size[t]
    assert C.sizeof(nat.BankItem) == -(-at // 8) * 8 == 40 == bankmod.ITEM_DTYPE.itemsize
    assert [bankmod.ITEM_DTYPE.fields[n][1] for _, n in fields] == [getattr(nat.BankItem, n).offset for _, n in fields]
    for name, v in (("NONE", 0), ("ENTRY", 1), ("WINDOW", 2)):
        assert re.search(rf"#define WW_BANK_NORM_{name} {v}\b", text) and getattr(nat, f"BANK_NORM_{name}") == v
    if shutil.which("gcc"):                                       # and the compiler's own word for it
        src = os.path.join(tmp_path, "s.c")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include "wakeword_amd.h"\nint main(void) { printf("%d\\n", (int)sizeof(ww_bank_item)); return 0; }\n')
        exe = os.path.join(tmp_path, "s")
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        assert int(subprocess.run([exe], capture_output=True, text=True, check=True).stdout) == 40


# ---- loader logic against a stand-in gather -------------------------------------------------------------------------------------
class _Proc:
    """The processor as the loader uses it: config, device, _check_augment, augment_batch, mel_batch."""
    config = pkg.AudioConfig
    device = None

    def __init__(self):
        self.calls = []

    def _check_augment(self):
        self.calls.append("check")

    def augment_batch(self, pcm):
        self.calls.append(("augment", random.random()))           # the plans are drawn here, after the batch's starts
        return pcm + 1.0

    def mel_batch(self, pcm, normalize=True):
        assert normalize is False
        return pcm[:, None, :80, None].repeat(1, 1, 1, 32).clone()


def _mixed_bank():
    proc = _Proc()
    b = pkg.ClipBank(proc)
    lens_a = np.array([N - 1, 3 * N, 0, N, N + 1], np.int64)        # clips; entry 2 is an unreadable placeholder
    b._add_segment(torch.zeros(int(lens_a.sum())), lens_a, bankmod.CLIP, [1, 1, 0, 0, 0], ok=[True, True, False, True, True],
                   peaks=np.ones(5, np.float32))
    lens_s = np.array([10 * N + 5, 100, 0], np.int64)               # streams: 11 windows, 1 window, none
    b._add_segment(torch.zeros(int(lens_s.sum())), lens_s, bankmod.STREAM, 0, peaks=np.ones(3, np.float32))
    b._add_segment(torch.zeros(2 * N + 2), [N + 1, N + 1], bankmod.CLIP, 1, peaks=np.ones(2, np.float32))
    seen = []

    def gather(entries, starts, norms, out=None, rows=None):
        seen.append((entries.copy(), starts.copy(), norms.copy()))
        return torch.from_numpy(np.repeat(entries[:, None].astype(np.float32), N, axis=1))
    b._gather = gather
    return b, proc, seen


def test_item_list_len_and_order():
    b, proc, _ = _mixed_bank()
    assert b.n_entries == 10 and b.unreadable == 1 and b.device == torch.device("cpu")
    items = b.item_entries()
    assert items.tolist() == [0, 1, 2, 3, 4, 8, 9] + [5] * 11 + [6]                  # clips in insertion order, then each stream's windows
    assert b.n_items == len(b) == 19
    assert b.nbytes == 4 * sum(s.numel() for s in b.segments) and b.hours == pytest.approx(float(b.lengths.sum()) / 16000 / 3600)
    assert "10 entries" in repr(b) and "19 items" in repr(b)
    ld = b.loader(4)
    assert len(ld) == 5 and ld.order() == list(range(19))
    ld = b.loader(4, drop_last=True)
    assert len(ld) == 4 and ld.order() == list(range(16))
    torch.manual_seed(3)
    want = torch.randperm(19).tolist()
    torch.manual_seed(3)
    assert b.loader(4, shuffle=True).order() == want
    with pytest.raises(ValueError):
        b.loader(0)
    assert proc.calls == []
    b.loader(4, augment=True)
    assert proc.calls == ["check"]                                                   # augment beyond 32 frames is refused there


@pytest.mark.parametrize("augment", [False, True])
def test_seeded_epoch_draws_exactly_the_starts_in_batch_order(augment):
    b, proc, seen = _mixed_bank()
    ld = b.loader(4, shuffle=True, augment=augment)
    random.seed(11)
    torch.manual_seed(11)
    out = list(ld)
    state = random.getstate()
    assert len(out) == 5 and [d.shape[0] for d, _ in out] == [4, 4, 4, 4, 3]
    # the replay: per batch, one randint per item whose entry is longer than N, in batch order; then the plans
    random.seed(11)
    torch.manual_seed(11)
    items = b.item_entries()[np.asarray(ld.order())]
    for k, (entries, starts, norms) in enumerate(seen):
        want_e = items[4 * k:4 * k + 4]
        assert entries.tolist() == want_e.tolist()
        want_s = [random.randint(0, int(b.lengths[e]) - N) if b.lengths[e] > N else 0 for e in want_e]
        assert starts.tolist() == want_s
        assert norms.tolist() == [nat.BANK_NORM_WINDOW if b.kinds[e] == bankmod.STREAM else nat.BANK_NORM_ENTRY for e in want_e]
        if augment:
            assert proc.calls[1 + k] == ("augment", random.random())
        data, target = out[k]
        assert data.shape == (len(want_e), 1, 80, 32) and target.shape == (len(want_e), 1) and target.dtype == torch.long
        assert target[:, 0].tolist() == b.labels[want_e].tolist()
        for r, e in enumerate(want_e):                              # placeholders are served as zeros, everything else as gathered
            assert torch.all(data[r] == (0.0 if not b.ok[e] else float(e) + (1.0 if augment else 0.0)))
    assert random.getstate() == state                               # and not one draw more


def test_no_draw_for_short_entries_and_placeholders():
    b, _, _ = _mixed_bank()
    random.seed(5)
    state = random.getstate()
    assert b.draw_starts(np.array([0, 2, 3, 6, 7])).tolist() == [0, 0, 0, 0, 0]      # N - 1, placeholder, N, 100, 0 samples
    assert random.getstate() == state
    s = b.draw_starts(np.array([4, 1]))
    random.setstate(state)
    assert s.tolist() == [random.randint(0, 1), random.randint(0, 2 * N)]


def test_gather_refuses_bad_arguments_before_any_device_call():
    b, _, seen = _mixed_bank()
    for bad in (dict(entries=[10]), dict(entries=[-1]), dict(entries=[0.5]), dict(entries=[0], starts=[N]), dict(entries=[0], starts=[-N - 1]),
                dict(entries=[0, 1], starts=[0]), dict(entries=[0], normalize="peak"), dict(entries=[0, 1], normalize=["entry"]),
                dict(entries=[0, 1], rows=[0, 0]), dict(entries=[0], rows=[1]), dict(entries=[0], out=torch.zeros(1, N - 1)),
                dict(entries=[0], out=torch.zeros(1, N, dtype=torch.float64))):
        with pytest.raises(ValueError):
            b.gather(**bad)
    assert seen == []
    b.gather([0, 1], starts=[N - 1, -N], normalize=[None, "window"])                 # the bounds are inclusive
    assert seen[0][1].tolist() == [N - 1, -N] and seen[0][2].tolist() == [0, 2]


def test_dataloader_routes_a_bank_to_its_loader():
    b, proc, _ = _mixed_bank()
    ld = pkg.DataLoader(b, batch_size=8, shuffle=True, num_workers=2, drop_last=True)
    assert isinstance(ld, bankmod.BankLoader) and (ld.batch_size, ld.shuffle, ld.drop_last, ld.augment) == (8, True, True, False)
    assert pkg.DataLoader(b, batch_size=8, augment=True).augment is True
    for kw in (dict(collate_fn=lambda x: x), dict(sampler=[0]), dict(batch_sampler=[[0]])):
        with pytest.raises(NotImplementedError):
            pkg.DataLoader(b, batch_size=8, **kw)
    with pytest.raises(NotImplementedError):
        pkg.DataLoader(b, batch_size=None)
    assert pkg.bank.ClipBank is pkg.ClipBank and hasattr(pkg.WakewordDataset, "cache")
