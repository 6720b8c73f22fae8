"""The size queries of every caller-owned workspace, and the guarded buffer the GPU tests use, on the CPU.

tests/test_gpu_workspaces.py hands each entry point a workspace of EXACTLY the queried size between guard bands; here the queries
themselves are checked (they are host arithmetic): non-decreasing in every size argument -- a short last batch must fit the block a
full batch was given -- and a multiple of 256 wherever the header asks for a 256-byte aligned workspace, so that regions carved from
the size stay aligned.  `Guarded` is tested on a CPU tensor: alignment, `intact()` after writes to the interior, and a one-byte write
into either guard is seen."""
import ctypes as C
import itertools
import json
import os

import pytest
import torch

from wakeword_jupyterlab_amd import _native as nat
from ws_harness import FILLS, GUARD_BYTE, Guarded

L = nat.lib
NS = (0, 1, 2, 5, 16, 17, 255, 256, 257, 4096)
WIDTHS = (1, 8, 31, 32, 33, 47, 48, 63)
SAMPLES = (4000, 4096, 8000, 12345, 16000, 16383, 16384, 24000, 32000)
AUG_SAMPLES = (4000, 4096, 8000, 12345, 16000, 16383)


def _table(sizes):
    tab = (nat.AdamTensor * len(sizes))()
    for k, n in enumerate(sizes):
        tab[k].p = tab[k].g = tab[k].m = tab[k].v = 4096 * (k + 1)         # never dereferenced by the query: non-null and 4-byte aligned
        tab[k].n = n
    return tab


def _grad_norm_bytes(n):
    return L.ww_grad_norm_workspace_bytes(_table([3, n + 1, 257]), 3)


# name -> (query taking one tuple of arguments, the grid of each argument, 256-byte multiple required by the header)
QUERIES = {
    "ww_cnn_scratch_bytes/3": (lambda n: L.ww_cnn_scratch_bytes(n, 3), (NS,), False),
    "ww_cnn_scratch_bytes/2": (lambda n: L.ww_cnn_scratch_bytes(n, 2), (NS,), False),
    "ww_cnn_wide_scratch_bytes/2": (lambda n, w: L.ww_cnn_wide_scratch_bytes(n, w, 2), (NS, WIDTHS), True),
    "ww_cnn_wide_scratch_bytes/3": (lambda n, w: L.ww_cnn_wide_scratch_bytes(n, w, 3), (NS, WIDTHS), True),
    "ww_workspace_bytes/2": (lambda n: L.ww_workspace_bytes(n, 2), (NS,), False),
    "ww_workspace_bytes/3": (lambda n: L.ww_workspace_bytes(n, 3), (NS,), False),
    "ww_workspace_frames_bytes/2": (lambda n, s: L.ww_workspace_frames_bytes(n, s, 2), (NS, SAMPLES), True),
    "ww_workspace_frames_bytes/3": (lambda n, s: L.ww_workspace_frames_bytes(n, s, 3), (NS, SAMPLES), True),
    "ww_forward_windows_workspace_bytes/2": (lambda n, s: L.ww_forward_windows_workspace_bytes(n, s, 2), (NS, SAMPLES), True),
    "ww_forward_windows_workspace_bytes/3": (lambda n, s: L.ww_forward_windows_workspace_bytes(n, s, 3), (NS, SAMPLES), True),
    "ww_events_workspace_bytes": (lambda n: L.ww_events_workspace_bytes(n), (NS + (5000,),), False),
    "ww_events_state_bytes": (lambda m, s: L.ww_events_state_bytes(m, s), ((1, 2, 5, 64, 65, 1000), (1, 2, 8, 255, 256)), False),
    "ww_train_workspace_bytes/2/f32": (lambda n: L.ww_train_workspace_bytes(n, 2, 0), (NS,), True),
    "ww_train_workspace_bytes/3/f32": (lambda n: L.ww_train_workspace_bytes(n, 3, 0), (NS,), True),
    "ww_train_workspace_bytes/2/f16x3": (lambda n: L.ww_train_workspace_bytes(n, 2, 1), (NS,), True),
    "ww_train_workspace_bytes/3/f16x3": (lambda n: L.ww_train_workspace_bytes(n, 3, 1), (NS,), True),
    "ww_augment_workspace_bytes": (lambda n: L.ww_augment_workspace_bytes(n), (NS,), True),
    "ww_augment_n_workspace_bytes": (lambda n, s: L.ww_augment_n_workspace_bytes(n, s), (NS, AUG_SAMPLES), True),
    "ww_augment_bg_workspace_bytes": (lambda n, s: L.ww_augment_bg_workspace_bytes(n, s), (NS, AUG_SAMPLES), True),
    "ww_augment_rir_workspace_bytes": (lambda n, s: L.ww_augment_rir_workspace_bytes(n, s), (NS, AUG_SAMPLES), True),
    "ww_mix_background_workspace_bytes": (lambda n: L.ww_mix_background_workspace_bytes(n), (NS,), True),
    "ww_reverb_workspace_bytes": (lambda n: L.ww_reverb_workspace_bytes(n), (NS,), True),
    "ww_rir_spectra_workspace_bytes": (lambda n: L.ww_rir_spectra_workspace_bytes(n), (NS,), True),
    "ww_bank_gather_workspace_bytes": (lambda n: L.ww_bank_gather_workspace_bytes(n), (NS,), True),
    "ww_bank_audit_workspace_bytes": (lambda t, n: L.ww_bank_audit_workspace_bytes(t, n), ((0, 1, 511, 512, 513, 70000, 1 << 20), NS), True),
    "ww_grad_norm_workspace_bytes": (_grad_norm_bytes, ((0, 1, 4092, 4093, 4094, 4096, 65536, 262145),), True),
}


@pytest.mark.parametrize("name", sorted(QUERIES))
def test_size_query_is_monotone_and_aligned(name):
    query, grids, aligned = QUERIES[name]
    values = {}
    for args in itertools.product(*grids):
        v = int(query(*args))
        assert v >= 0, f"{name}{args}: error code {v} ({(L.ww_last_error() or b'').decode()})"
        if aligned:
            assert v % 256 == 0, f"{name}{args} = {v}: not a multiple of 256"
        values[args] = v
    for args, v in values.items():
        for axis, grid in enumerate(grids):
            i = grid.index(args[axis])
            if i + 1 < len(grid):
                up = args[:axis] + (grid[i + 1],) + args[axis + 1:]
                assert values[up] >= v, f"{name}: {up} needs {values[up]} bytes, fewer than {args} ({v})"


def test_forward_size_queries_agree_and_are_the_recorded_ones():
    """One layout serves the forward path: ww_workspace_frames_bytes and ww_forward_windows_workspace_bytes are equal at every clip
    length, and at one second both equal ww_workspace_bytes.  Each also equals the size recorded from the library of the commit before
    the layouts were folded into one (tests/golden/forward_workspace_sizes.json, written by make_forward_workspace_sizes.py)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_workspace_sizes.json")) as f:
        recorded = json.load(f)
    assert {k: len(v) for k, v in recorded.items()} == {"ww_workspace_bytes": len(NS) * 2, "ww_workspace_frames_bytes": len(NS) * len(SAMPLES) * 2,
                                                        "ww_forward_windows_workspace_bytes": len(NS) * len(SAMPLES) * 2}
    for n, s, c in itertools.product(NS, SAMPLES, (2, 3)):
        frames, windows = L.ww_workspace_frames_bytes(n, s, c), L.ww_forward_windows_workspace_bytes(n, s, c)
        assert frames == windows, (n, s, c, frames, windows)
        assert frames == recorded["ww_workspace_frames_bytes"][f"{n},{s},{c}"], (n, s, c)
        assert windows == recorded["ww_forward_windows_workspace_bytes"][f"{n},{s},{c}"], (n, s, c)
        if s == 16000:
            assert L.ww_workspace_bytes(n, c) == frames == recorded["ww_workspace_bytes"][f"{n},{c}"], (n, c)


def test_augment_layout_tiles_the_queried_size():
    """The regions of ww_augment_workspace_layout are 256-byte aligned, in order, disjoint, and end at the queried size; the records
    region is the first one (the GPU test poisons everything behind it)."""
    for n, s in itertools.product((1, 5, 17), AUG_SAMPLES):
        lay = nat.AugmentLayout()
        assert L.ww_augment_workspace_layout(n, s, C.byref(lay)) == 0
        assert lay.total_bytes == L.ww_augment_n_workspace_bytes(n, s)
        assert lay.record_bytes == L.ww_augment_record_bytes()
        offs = [lay.records, lay.buf_a, lay.buf_b, lay.spec, lay.y, lay.total_bytes]
        sizes = [n * lay.record_bytes, n * lay.row_bytes, n * lay.row_bytes, n * lay.spec_clip_bytes, n * lay.y_clip_bytes]
        assert offs[0] == 0 and all(o % 256 == 0 for o in offs)
        for a, b, size in zip(offs, offs[1:], sizes):
            assert a + size <= b, (n, s, offs, sizes)
        assert L.ww_augment_bg_workspace_bytes(n, s) >= lay.total_bytes and L.ww_augment_rir_workspace_bytes(n, s) >= L.ww_augment_bg_workspace_bytes(n, s)


# ---- the harness itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [0, 1, 255, 256, 257, 4099])
@pytest.mark.parametrize("align", [16, 256])
@pytest.mark.parametrize("fill", FILLS)
def test_guarded_interior_is_aligned_exact_and_filled(nbytes, align, fill):
    g = Guarded(nbytes, fill, align=align, device="cpu")
    assert g.ptr % align == 0 and g.interior.numel() == nbytes and g.ptr == g.raw.data_ptr() + g.start
    assert nbytes == 0 or g.interior.data_ptr() == g.ptr                   # (torch reports no address for an empty view)
    assert g.raw.numel() >= 4096 + nbytes + 4096 and g.start >= 4096 and g.raw.numel() - g.start - nbytes >= 4096
    assert bool((g.interior == fill).all()) and g.intact() and not g.touched()
    assert bool((g.raw[:g.start] == GUARD_BYTE).all()) and bool((g.raw[g.start + nbytes:] == GUARD_BYTE).all())


def test_guarded_sees_writes_to_the_interior_only_as_touched():
    g = Guarded(1000, 0xFF, device="cpu")
    g.interior[0] = 0
    g.interior[999] = 7
    g.view(torch.float32, (250,))[3] = 1.5
    assert g.intact() and g.touched()
    g.refill()
    assert g.intact() and not g.touched()
    g.refill(0x00, start=100)
    assert g.touched(start=100) and bool((g.interior[:100] == 0xFF).all()) and bool((g.interior[100:] == 0x00).all())


@pytest.mark.parametrize("nbytes", [0, 1, 1000, 4096])
def test_a_one_byte_write_into_either_guard_is_detected(nbytes):
    for where in ("first past the end", "last before the start", "far end", "far start"):
        g = Guarded(nbytes, 0x00, device="cpu")
        index = {"first past the end": g.start + nbytes, "last before the start": g.start - 1, "far end": g.raw.numel() - 1, "far start": 0}[where]
        assert g.intact()
        g.raw[index] = GUARD_BYTE ^ 0x01                                   # one bit of one byte
        assert not g.intact(), where
        g.raw[index] = GUARD_BYTE
        assert g.intact()


def test_typed_output_views_end_at_the_guard():
    g = Guarded.for_output((5, 2), torch.float32, device="cpu")
    v = g.view()
    assert v.shape == (5, 2) and v.dtype == torch.float32 and v.data_ptr() == g.ptr and g.nbytes == 40
    assert torch.isnan(v).all()                                            # 0xFF is a NaN as float32 ...
    assert bool((g.view(torch.int64, (5,)) == -1).all())                   # ... and -1 as an integer
    assert bool(torch.isnan(Guarded.for_output((3,), torch.float64, device="cpu").view()).all())
    v.zero_()
    assert g.intact()
    one_short = g.raw[g.start + 4:g.start + 4 + 40].view(torch.float32)   # the same output backed one element late: its last element is guard
    one_short.zero_()
    assert not g.intact()
    with pytest.raises(ValueError):
        g.view(torch.float32, (11,))
    h = Guarded.holding(torch.arange(7, dtype=torch.int64))
    assert torch.equal(h.view(), torch.arange(7, dtype=torch.int64)) and h.intact() and h.nbytes == 56
