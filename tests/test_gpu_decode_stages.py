"""K0 (csrc/ww_decode.hip: decode_resample_kernel, resample_lds_kernel) stage by stage against float64 ON ITS OWN INPUT.

ww_decode_resample_n runs on descriptors built in memory (no files); many descriptors per launch.  Bounds (u = 2^-24), all derived in
oracle/decode_oracle.py and tests/test_host_decode_stages.py, none measured:

  conversion, 1 channel     equality with float32(v scale)
  conversion, C channels    |mono - mean| <= C u mean|v|; and K0's channel sum is sequential float32 (s += v over the channels in order,
                            then / float(C)): asserted bit for bit against that restatement
  resample, own input       |got[j] - y[j]| <= n[j] u A[j] + 2^-149, y the float64 sum over K0's float32 mono and K0's float32 taps
  definition                |got[j] - resample_poly(float64(mono))[j]| <= the above + 6e-8 max(1, up) sum |x| over the output's frames
  normalise                 valid samples == float32(row / peak) bit for bit, peak = max |row| of the unnormalised GPU run of the same
                            file; 0.0 past n_out - crop_start; a silent file NaN in the valid part
  bit-identities            windowed form == whole-file form; vector path == general loop; batch == alone; LDS form == direct form (both
                            equal the direct form's fma chain emulated bit for bit on the CPU, oracle fma_chain_f32)

Measured on the MI355X (scripts/decode_stage_errors.py -> profiles/k0_stage_errors.json): the largest |got - y| / (n u A) over the
fifteen rates is 0.50 (1 kHz, at outputs of a single product, whose one rounding may use all of u |x h|; 0.43 at 6 kHz, 0.32 and less
from 7.35 kHz up, where the chains are longer); every rate's rows equal the emulated fma chain bit for bit.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
from scipy.signal import resample_poly

import k0_cases as k0
from oracle import decode_oracle as do
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd.files import DESC_DTYPE

pytestmark = pytest.mark.gpu
FIGURES = []


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _figures_file():
    yield
    path = os.environ.get("WW_K0_STAGE_JSON")
    if path and FIGURES:
        with open(path, "w") as f:
            json.dump(FIGURES, f, indent=1)


_PROTO = {}


def _descs(pack):
    d = np.zeros(len(pack.descs), dtype=DESC_DTYPE)
    for i, (off, n_frames, ch, sr, fmt, crop) in enumerate(pack.descs):
        if sr not in _PROTO:
            p = nat.ClipDesc()
            nat.check(nat.lib.ww_resampler_prepare(sr, C.byref(p)))
            _PROTO[sr] = (p.up, p.down, p.half_len, p.taps_dev or 0)
            assert _PROTO[sr][:3] == k0.taps(sr)[1:] if sr != 16000 else _PROTO[sr][:2] == (1, 1)     # (16 kHz: no filter, half_len unused)
        up, down, hl, taps_dev = _PROTO[sr]
        d[i] = (off, n_frames, ch, sr, fmt, crop, up, down, hl, 0, taps_dev)
    return d


def run_k0(dev, pack, normalize, row_len, alone=False):
    """One launch over all of the pack's descriptors (alone: one launch per descriptor) into rows pre-filled with 7.0, with a guard row in
    front and behind that must come back untouched."""
    d = _descs(pack)
    n = len(d)
    raw_dev = torch.from_numpy(pack.raw()).to(dev)
    descs_dev = torch.from_numpy(d.view(np.uint8).reshape(n, DESC_DTYPE.itemsize).copy()).to(dev)
    out = torch.full((n + 2, row_len), 7.0, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    step = out.stride(0) * 4
    for i in (range(n) if alone else (0,)):
        nat.check(nat.lib.ww_decode_resample_n(C.c_void_p(raw_dev.data_ptr()), C.c_void_p(descs_dev.data_ptr() + i * DESC_DTYPE.itemsize),
                                               1 if alone else n, normalize, row_len, C.c_void_p(out.data_ptr() + (i + 1) * step), stream))
    o = out.cpu().numpy()
    assert (o[0] == 7.0).all() and (o[-1] == 7.0).all(), "K0 wrote outside its rows"
    return o[1:-1]


def _check_stage(got, y, A, n, x32, sr, what):
    """got (float32, unnormalised, whole file) against the own-input oracle and the definition; returns the share of the bound used."""
    t, up, down, hl = k0.taps(sr)
    err = np.abs(got.astype(np.float64) - y)
    bound = do.stage_bound(A, n)
    ratio = float((err / bound).max())
    ref = resample_poly(x32.astype(np.float64), up, down)
    err_def = np.abs(got.astype(np.float64) - ref)
    bound_def = bound + do.TAP_TOL * max(1, up) * do.frames_abs_sum(x32, up, down, hl)
    print(f"{what}: max |got - y| {err.max():.3e} = {ratio:.3f} of n u A (n <= {n.max()});  max |got - resample_poly| {err_def.max():.3e}")
    assert (err <= bound).all(), (what, ratio)
    assert (err_def <= bound_def).all(), (what, float((err_def / bound_def).max()))
    return ratio, float(err_def.max())


def _window(whole, crop, row_len):
    w = np.zeros(row_len, np.float32)
    v = whole[crop:crop + row_len]
    w[:len(v)] = v
    return w, len(v)


def _normalised(whole, crop, row_len):
    w, v = _window(whole, crop, row_len)
    peak = np.float32(np.abs(whole).max()) if len(whole) else np.float32(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        w[:v] = w[:v] / peak                                     # float32 / float32, correctly rounded, as the kernel's division
    return w


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("sr", k0.RATES)
def test_rate_every_edge_length_crop_and_row_length(dev, sr):
    t, up, down, hl = k0.taps(sr)
    files = []                                                   # (offset, n_frames, x32, y, A, n)
    pack0 = k0.Pack()
    for n_in in k0.frame_counts(sr):
        codes = k0.noise_s16(n_in, 1000 + n_in)
        _, x32 = do.mono_f64(codes, do.FMT_S16, 1)
        files.append((pack0.add_bytes(k0.to_bytes(codes, do.FMT_S16)), n_in, x32) + do.resample_own_input(x32, t, up, down, hl))
    zero_off, zero_n = pack0.add_bytes(np.zeros(2 * 500, np.uint8)), 500
    nonzero, worst, worst_def, chain_equal = 0, 0.0, 0.0, True
    for row_len in k0.ROW_LENS:
        pack = k0.Pack()
        pack.chunks, pack.size = list(pack0.chunks), pack0.size
        plan = []                                                # (file index or None, crop, is a cover window)
        for f, (off, n_in, x32, y, A, n) in enumerate(files):
            n_out = len(y)
            covers = list(range(0, n_out, row_len))
            for crop in covers + [c for c in k0.crops(n_out, sr, row_len) if c not in covers]:
                pack.desc(off, n_in, 1, sr, do.FMT_S16, crop)
                plan.append((f, crop, crop in covers))
        for crop in (0, 1):
            pack.desc(zero_off, zero_n, 1, sr, do.FMT_S16, crop)
            plan.append((None, crop, False))
        rows0 = run_k0(dev, pack, 0, row_len)
        rows1 = run_k0(dev, pack, 1, row_len)
        whole = {}
        for f, (off, n_in, x32, y, A, n) in enumerate(files):
            parts = [rows0[i] for i, (ff, crop, cover) in enumerate(plan) if ff == f and cover]
            cat = np.concatenate(parts)
            assert not cat[len(y):].any()                        # the zero pad behind the file's last output
            whole[f] = cat[:len(y)]
            ratio, e_def = _check_stage(whole[f], y, A, n, x32, sr, f"{sr} Hz {n_in} frames rows of {row_len}")
            worst, worst_def = max(worst, ratio), max(worst_def, e_def)
            if len(y) <= 4100 and row_len == k0.ROW_LENS[0]:
                chain_equal = chain_equal and np.array_equal(whole[f], do.fma_chain_f32(x32, t, up, down, hl))
        n_zero_out = k0.n_out_of(zero_n, sr)
        for i, (f, crop, cover) in enumerate(plan):
            if f is None:
                assert not rows0[i].any()
                v = max(0, min(row_len, n_zero_out - crop))
                assert np.isnan(rows1[i][:v]).all() and v > 0 and not rows1[i][v:].any()     # 0 / 0 in the valid part, 0.0 in the padding
                continue
            w, v = _window(whole[f], crop, row_len)
            assert np.array_equal(rows0[i], w), (sr, files[f][1], crop, row_len)             # windowed form == whole-file form
            assert _same(rows1[i], _normalised(whole[f], crop, row_len)), (sr, files[f][1], crop, row_len)
            nonzero += int(np.count_nonzero(w)) + int(np.count_nonzero(rows1[i]))
    assert nonzero > 0 and chain_equal
    FIGURES.append({"rate": sr, "up": up, "down": down, "taps": 2 * hl + 1, "kernel": "lds" if k0.in_lds(sr) else "direct",
                    "max_ratio_of_n_u_A": worst, "max_products": int(max(f[5].max() for f in files)),
                    "max_abs_err_vs_resample_poly": worst_def, "rows_equal_emulated_fma_chain": bool(chain_equal)})


def _codes(fmt, n_frames, ch, seed):
    """Random samples of the format over its whole range; the first frames hold its extreme codes (most negative, most positive, -1, 0),
    once the same in every channel and once rotated through the channels."""
    rng = np.random.default_rng(seed)
    if fmt in (do.FMT_F32, do.FMT_F64):
        v = rng.uniform(-1.0, 1.0, size=(n_frames, ch))
        v = v.astype(np.float32).astype(np.float64) if fmt == do.FMT_F32 else v
        ext = [-1.0, 1.0 - 2.0 ** -24, -(2.0 ** -126), 0.0] if fmt == do.FMT_F32 else [-1.0, 1.0 - 2.0 ** -30, -(2.0 ** -60), 0.0, 1 / 3]
    else:
        lo, hi = {do.FMT_S16: (-32768, 32767), do.FMT_U8: (0, 255), do.FMT_S24: (-(1 << 23), (1 << 23) - 1),
                  do.FMT_S32: (-(1 << 31), (1 << 31) - 1)}[fmt]
        v = rng.integers(lo, hi + 1, size=(n_frames, ch), dtype=np.int64)
        ext = [lo, hi, 127 if fmt == do.FMT_U8 else -1, 128 if fmt == do.FMT_U8 else 0]
    for k, e in enumerate(ext):
        v[k, :] = e
        v[len(ext) + k, :] = [ext[(k + c) % len(ext)] for c in range(ch)]
    return v.reshape(-1)


@pytest.mark.parametrize("fmt", [do.FMT_S16, do.FMT_U8, do.FMT_S24, do.FMT_S32, do.FMT_F32, do.FMT_F64], ids=["s16", "u8", "s24", "s32", "f32", "f64"])
def test_conversion_and_mono_of_every_format_and_channel_count(dev, fmt):
    pack, plan = k0.Pack(), []
    for sr, n_frames in ((16000, 1003), (48000, 3010)):
        for ch in (1, 2, 3, 8):
            codes = _codes(fmt, n_frames, ch, 10 * fmt + ch)
            b = k0.to_bytes(codes, fmt)
            held = do.codes_from_bytes(b, fmt)                    # what the bytes hold (float32 files: the rounded samples)
            pack.desc(pack.add_bytes(b), n_frames, ch, sr, fmt, 0)
            plan.append((sr, ch, held))
    rows = run_k0(dev, pack, 0, 16000)
    nonzero = 0
    for row, (sr, ch, held) in zip(rows, plan):
        m64, m32 = do.mono_f64(held, fmt, ch)
        if sr == 16000:
            got = row[:len(m64)]
            assert not row[len(m64):].any()
            if ch == 1:
                assert np.array_equal(got, m64.astype(np.float32)) and np.array_equal(m64, m32.astype(np.float64))
            else:
                v = np.abs(do.mono_f64(np.asarray(held).reshape(-1), fmt, 1)[0]).reshape(-1, ch)
                assert (np.abs(got.astype(np.float64) - m64) <= ch * do.U32 * v.mean(axis=1)).all(), (fmt, ch)
                assert np.array_equal(got, m32), (fmt, ch)        # the sequential float32 sum, then one division
        else:
            t, up, down, hl = k0.taps(sr)
            y, A, n = do.resample_own_input(m32, t, up, down, hl)
            got = row[:len(y)]
            assert not row[len(y):].any()
            _check_stage(got, y, A, n, m32, sr, f"format {fmt} x {ch} channels at {sr} Hz")
        nonzero += int(np.count_nonzero(got))
    assert nonzero > 0


@pytest.mark.parametrize("normalize", [0, 1])
def test_16k_s16_mono_vector_path_and_its_partial_last_vector(dev, normalize):
    """16 kHz mono S16 of at most 16000 frames at a 16-byte boundary takes the eight-samples-per-load path; the same samples at a byte
    offset of 2 mod 16 take the general loop; 16001 frames leave the vector path at any alignment.  All exact, and bit-identical."""
    counts = (0, 1, 7, 8, 9, 2047, 15999, 16000, 16001)
    pack, codes = k0.Pack(), {}
    for n in counts:
        codes[n] = k0.noise_s16(n, 50 + n) if n else np.zeros(0, np.int64)
        for shift in (0, 2):
            off = pack.add_bytes(k0.to_bytes(codes[n], do.FMT_S16), shift)
            assert off % 16 == shift
            pack.desc(off, n, 1, 16000, do.FMT_S16, 0)
    rows = run_k0(dev, pack, normalize, 16000)
    nonzero = 0
    for k, n in enumerate(counts):
        whole = (codes[n] * 2.0 ** -15).astype(np.float32)
        want = _normalised(whole, 0, 16000) if normalize else _window(whole, 0, 16000)[0]
        assert np.array_equal(rows[2 * k], want), n               # aligned: the vector path (n <= 16000)
        assert np.array_equal(rows[2 * k + 1], rows[2 * k]), n    # 2 mod 16: the general loop
        nonzero += int(np.count_nonzero(want))
        if normalize and n:
            assert np.abs(rows[2 * k][:min(n, 16000)]).max() == 1.0 or n > 16000
    assert nonzero > 0


@pytest.mark.parametrize("sr", [44100, 96000, 11025])
def test_windows_of_a_3s_file_are_the_whole_file_and_the_fma_chain_bit_for_bit(dev, sr):
    """normalize = 0 starts its blocks at crop_start, normalize = 1 at output 0: every output must not depend on where its block starts
    (44.1 kHz, 96 kHz: resample_lds_kernel; 11.025 kHz: decode_resample_kernel's direct form).  The normalised rows are compared after the
    division, which is all a caller can see: float32(window / peak) with the window and the peak from the unnormalised runs.  And the
    whole file equals the direct form's fma chain emulated on the CPU, so the LDS form equals the direct form."""
    t, up, down, hl = k0.taps(sr)
    n_in = 3 * sr
    codes = k0.noise_s16(n_in, sr)
    _, x32 = do.mono_f64(codes, do.FMT_S16, 1)
    n_out = k0.n_out_of(n_in, sr)
    assert n_out == 48000
    crops = [0, 16000, 32000, 1, 2047, 2048, 2049, n_out - 16000]
    pack = k0.Pack()
    off = pack.add_bytes(k0.to_bytes(codes, do.FMT_S16))
    for c in crops:
        pack.desc(off, n_in, 1, sr, do.FMT_S16, c)
    rows0, rows1 = run_k0(dev, pack, 0, 16000), run_k0(dev, pack, 1, 16000)
    whole = np.concatenate(rows0[:3])
    for row0, row1, c in zip(rows0, rows1, crops):
        assert np.array_equal(row0, whole[c:c + 16000]), c
        assert np.array_equal(row1, _normalised(whole, c, 16000)), c
    assert np.count_nonzero(whole) > 40000
    y, A, n = do.resample_own_input(x32, t, up, down, hl)
    _check_stage(whole, y, A, n, x32, sr, f"{sr} Hz 3 s")
    assert np.array_equal(whole, do.fma_chain_f32(x32, t, up, down, hl))


def test_1100_interleaved_descriptors_in_one_launch_equal_each_alone(dev):
    """More than twice resample_lds_kernel's grid (2 x the CU count), so every workgroup takes several clips, and consecutive clips of a
    workgroup change filter: 48 k, 44.1 k, 16 k, 11.025 k, 8 k, an undecoded FLAC descriptor, repeated.  Some files have no frames."""
    n_desc = 1100
    assert n_desc > 2 * 2 * torch.cuda.get_device_properties(dev).multi_processor_count
    rates = (48000, 44100, 16000, 11025, 8000, 16000)
    noise = np.random.default_rng(8).integers(-32768, 32768, size=40000, dtype=np.int64)
    pack = k0.Pack()
    off = pack.add_bytes(k0.to_bytes(noise, do.FMT_S16))
    empty = []
    for i in range(n_desc):
        sr, flac = rates[i % 6], i % 6 == 5
        n = 0 if i % 50 == 7 else 150 + (i * 37) % 500
        start = (i * 61) % 30000
        pack.desc(off + 2 * start, n, 1, sr, nat.FMT_FLAC if flac else do.FMT_S16, crop_start=(i % 3) * 5 if not flac else 0)
        empty.append(flac or n == 0)
    for normalize in (1, 0):
        batch = run_k0(dev, pack, normalize, 4000)
        alone = run_k0(dev, pack, normalize, 4000, alone=True)
        assert _same(batch, alone)
        for i in range(n_desc):
            assert empty[i] == (not batch[i].any()), i             # zero rows for skipped and zero-length files, over the 7.0 pre-fill
        assert np.isfinite(batch).all() and np.count_nonzero(batch) > 100000
    # one row against the oracle, so that "equal" is not "equally wrong": descriptor 1 (44.1 kHz), unnormalised
    t, up, down, hl = k0.taps(44100)
    o, n, ch, sr, fmt, crop = pack.descs[1]
    _, x32 = do.mono_f64(noise[(o - off) // 2:(o - off) // 2 + n], do.FMT_S16, 1)
    y, A, nn = do.resample_own_input(x32, t, up, down, hl)
    assert (np.abs(batch[1][:len(y) - crop] - y[crop:]) <= do.stage_bound(A, nn)[crop:]).all() and not batch[1][len(y) - crop:].any()


def _k0_path(desc, row_len):
    """The branch of decode_resample_kernel a descriptor takes (csrc/ww_decode.hip), from the descriptor alone."""
    off, n, ch, sr, fmt, crop = desc
    if sr != 16000 and k0.in_lds(sr):
        return f"resample_lds_kernel's ({sr})"
    if fmt == nat.FMT_FLAC:
        return "skipped FLAC"
    if n == 0:
        return "zero frames"
    if sr != 16000:
        return f"direct taps ({sr})"
    if row_len == 16000 and ch == 1 and fmt == do.FMT_S16 and n <= 16000 and crop == 0 and off % 16 == 0:
        return "16 k vector path"
    return "16 k general loop"


_GRID_KINDS = (48000, 44100, "16 k aligned", 11025, 8000, "flac", "16 k general", "empty")


def _grid_pack(n_cu):
    """2 x 8 x CUs + 77 tiny files in one pack: the rates, the undecoded FLAC descriptor and the empty files of the 1100-descriptor test,
    keyed so that the interleave cannot alias decode_resample_kernel's grid g = 8 x CUs: descriptor i = q g + r is of kind
    (r + q d) % 8 with d = 1 + (r // 8) % 7, so the next clip of a workgroup (i + g) is d kinds on -- never the same kind, and over r
    every kind precedes every other.  16 kHz files come in two kinds: 16-byte aligned with crop 0 (the vector path at rows of 16000) and
    at an odd sample with a crop (the general loop); "empty" is a 16 kHz file of no frames (and a few of resample_lds_kernel's files are empty)."""
    g = 8 * n_cu
    noise = np.random.default_rng(8).integers(-32768, 32768, size=40000, dtype=np.int64)
    pack = k0.Pack()
    off = pack.add_bytes(k0.to_bytes(noise, do.FMT_S16))
    assert off % 16 == 0
    for i in range(2 * g + 77):
        q, r = divmod(i, g)
        kind = _GRID_KINDS[(r + q * (1 + (r // 8) % 7)) % 8]
        lds_empty = kind in (48000, 44100, 8000) and (r + 3 * q) % 50 == 7       # resample_lds_kernel's own empty files
        n = 0 if kind == "empty" or lds_empty else 150 + (i * 37) % 500
        start = (i * 64) % 30000                                  # a multiple of 8 samples: 16-byte aligned
        if kind == "16 k aligned":
            pack.desc(off + 2 * start, n, 1, 16000, do.FMT_S16, crop_start=0)
        elif kind == "16 k general":
            pack.desc(off + 2 * (start + 1), n, 1, 16000, do.FMT_S16, crop_start=(i % 3) * 5)
        elif kind in ("flac", "empty"):
            pack.desc(off + 2 * start, n, 1, 16000, nat.FMT_FLAC if kind == "flac" else do.FMT_S16, crop_start=0)
        else:
            pack.desc(off + 2 * (start + i % 2), n, 1, kind, do.FMT_S16, crop_start=(i % 3) * 5)
    return pack, noise, off


def _check_grid_paths(pack, n_cu, row_len):
    """Consecutive clips of a decode_resample_kernel workgroup (c, then c + g) never take the same branch, and each of the kernel's own
    branches is entered right after, and right before, each other one.  (Rows of 4000 have no vector path: there the two 16 kHz kinds
    share the general loop.)  -> the path of every descriptor"""
    g = 8 * n_cu
    n_desc = len(pack.descs)
    assert n_desc > 2 * g
    paths = [_k0_path(d, row_len) for d in pack.descs]
    pairs = {(paths[c], paths[c + g]) for c in range(n_desc - g)}
    same = {a for a, b in pairs if a == b}
    assert same <= (set() if row_len == 16000 else {"16 k general loop"}), same
    own = ["16 k general loop", "skipped FLAC", "zero frames", "direct taps (11025)"] + (["16 k vector path"] if row_len == 16000 else [])
    missing = [(a, b) for a in own for b in own if a != b and (a, b) not in pairs]
    assert not missing, missing
    lds = sorted({p for p in paths if p.startswith("resample_lds")})
    assert len(lds) == 3 and all((a, b) in pairs and (b, a) in pairs for a in lds for b in own), "a skipped descriptor before and after each branch"
    return paths


@pytest.mark.parametrize("row_len", [4000, 16000])
def test_descriptors_beyond_the_resident_grid_of_both_kernels(dev, row_len):
    """test_1100_interleaved_descriptors...'s sibling for decode_resample_kernel, whose grid is 8 per CU: at 1100 descriptors its
    workgroups take one clip each, and its red[], its early `continue`s and the vector path's own barriers are never handed from clip
    to clip.  Here 2 x 8 x CUs + 77 descriptors (_grid_pack): every workgroup of decode_resample_kernel enters its second iteration and
    77 their third (resample_lds_kernel, 2 per CU, takes eight or nine; its order is not controlled here).  Rows of 4000 as in the
    sibling, and rows of 16000, without which the vector path of 16 kHz files cannot be taken.  Batch == launches of at most one clip
    per CU (grid = n: no second iteration), bit for bit, for both `normalize` values; one row per path against the oracle."""
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    g = 8 * n_cu
    pack, noise, off = _grid_pack(n_cu)
    n_desc = len(pack.descs)
    assert n_desc == 2 * g + 77
    paths = _check_grid_paths(pack, n_cu, row_len)               # before any launch

    def chunked(normalize):
        parts = []
        for c in range(0, n_desc, n_cu):
            sub = k0.Pack()
            sub.chunks, sub.size, sub.descs = pack.chunks, pack.size, pack.descs[c:c + n_cu]
            parts.append(run_k0(dev, sub, normalize, row_len))
        return np.concatenate(parts)

    for normalize in (1, 0):
        batch = run_k0(dev, pack, normalize, row_len)
        assert _same(batch, chunked(normalize))
        empty = np.array([d[4] == nat.FMT_FLAC or d[1] == 0 for d in pack.descs])
        assert np.array_equal(empty, ~batch.any(axis=1))          # zero rows for skipped and zero-length files, over the 7.0 pre-fill
        assert np.isfinite(batch).all() and np.count_nonzero(batch) > 100000
    # one unnormalised row per path against the oracle, so that "equal" is not "equally wrong": each a second or third clip of its workgroup
    for want in sorted(set(paths) - {"skipped FLAC", "zero frames"}):
        i = next(i for i in range(g, n_desc) if paths[i] == want and pack.descs[i][1] > 0)
        o, n, ch, sr, fmt, crop = pack.descs[i]
        _, x32 = do.mono_f64(noise[(o - off) // 2:(o - off) // 2 + n], do.FMT_S16, 1)
        if sr == 16000:                                          # no filter: the converted samples themselves
            assert np.array_equal(batch[i][:n - crop], x32[crop:]) and not batch[i][n - crop:].any(), (want, i)
            continue
        t, up, down, hl = k0.taps(sr)
        y, A, nn = do.resample_own_input(x32, t, up, down, hl)
        assert (np.abs(batch[i][:len(y) - crop] - y[crop:]) <= do.stage_bound(A, nn)[crop:]).all() and not batch[i][len(y) - crop:].any(), (want, i)


def test_normalise_takes_the_peak_of_the_whole_file(dev):
    """The peak outside the crop window; a crop whose valid part is shorter than the row; silent files on all three code paths (LDS form,
    general loop, vector path): NaN in the valid part -- the reference divides by max|x| = 0 -- and 0.0 in the padding."""
    pack, plan = k0.Pack(), []
    for sr in (48000, 16000, 11025):
        n_in = int(1.5 * sr)
        codes = np.random.default_rng(sr).integers(-4000, 4001, size=n_in, dtype=np.int64)
        codes[-sr // 10:] *= 8                                    # the loud last tenth of a second
        codes[0], codes[-1] = 100, -32000
        off = pack.add_bytes(k0.to_bytes(codes, do.FMT_S16))
        n_out = k0.n_out_of(n_in, sr) if sr != 16000 else n_in
        for crop in (0, 3, n_out - 16000, n_out - 5000, n_out - 1):
            pack.desc(off, n_in, 1, sr, do.FMT_S16, crop)
            plan.append((sr, codes, n_out, crop))
    silent = pack.add_bytes(np.zeros(2 * 24000, np.uint8))
    for sr, n, crop in ((48000, 24000, 0), (48000, 24000, 7000), (11025, 3000, 0), (16000, 9000, 0), (16000, 9000, 100), (16000, 20000, 5000)):
        pack.desc(silent, n, 1, sr, do.FMT_S16, crop)
        plan.append((sr, None, k0.n_out_of(n, sr) if sr != 16000 else n, crop))
    rows0, rows1 = run_k0(dev, pack, 0, 16000), run_k0(dev, pack, 1, 16000)
    whole = {}
    for i, (sr, codes, n_out, crop) in enumerate(plan):
        v = min(16000, n_out - crop)
        if codes is None:
            assert not rows0[i].any() and np.isnan(rows1[i][:v]).all() and not rows1[i][v:].any() and 0 < v
            continue
        if crop == 0:
            assert n_out <= 32000
            whole[sr] = np.concatenate([rows0[i], rows0[i + 2][32000 - n_out:]])    # crops 0 and n_out - 16000 cover the file
            assert len(whole[sr]) == n_out
            peak = np.abs(whole[sr]).max()
            assert np.abs(whole[sr][:16003]).max() < 0.5 * peak                     # the peak is outside the first windows
        assert np.array_equal(rows0[i], _window(whole[sr], crop, 16000)[0])
        assert np.array_equal(rows1[i], _normalised(whole[sr], crop, 16000)), (sr, crop)
        assert np.count_nonzero(rows1[i][:v]) > 0 and not rows1[i][v:].any()
        if crop == 0:
            assert np.abs(rows1[i]).max() < 0.5
