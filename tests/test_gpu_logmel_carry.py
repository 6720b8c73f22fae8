"""The clip loop of the persistent log-mel kernels BEYOND their resident grids (csrc/ww_logmel.hip).

Each kernel launches min(n, CUs x blocks-per-CU) workgroups, and a workgroup walks clip, clip + grid, ...: the mel tile, red[], the
auto-mode flag words and the sample prefetch chain (rs_next) of one clip are the next clip's.  The other log-mel tests stay at or
under 300 clips, where on a 256-CU part every float workgroup takes exactly one clip.  Here B = 2 x 3 x CUs + 41 rows:

  logmel_kernel<., 4, 32>   grid 3 x CUs   1 s clips, f32 and auto            every workgroup takes 2 clips, 41 take 3
  logmel_kernel<., 4, 64>   grid 2 x CUs   every other length, f32 and auto   3 clips each, 41 take 4
  logmel64_kernel<., 32>    grid 2 x CUs   1 s clips, f64 and auto's redo     3 and 4
  logmel64_kernel<., 64>    grid 1 x CUs   every other length                 6 and 7

and logmel_cases.carry_batch orders the rows so that inside a workgroup of every one of these grids each kind of clip (noisy, noise-free
and therefore marked in auto mode, NaN / Inf, silent, loud) directly follows each kind.  The 8-wave instances never loop (their grid is
n <= CUs): they give the reference, one clip per workgroup.  Everything is bit equality or the project's MEL_TOL against the oracle.
"""
import functools

import numpy as np
import pytest
import torch

import logmel_cases as lc
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import ops
from wakeword_jupyterlab_amd.config import AudioConfig

pytestmark = pytest.mark.gpu

MEL_TOL = 1e-4
MATHS = ["f32", "f64", "auto"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def n_cu(dev):
    n = torch.cuda.get_device_properties(dev).multi_processor_count
    # the widest resident grid is K1Layout<4, 32>::kBlocksPerCu = 3 per CU (K1Layout<4, 64>::kBlocksPerCu and K64Layout<32>::kBlocksPerCu
    # are 2, K64Layout<64>::kBlocksPerCu is 1): a change there must be followed in logmel_cases.CARRY_GRIDS_PER_CU
    assert lc.carry_rows(n) > 2 * 3 * n
    return n


@functools.lru_cache(maxsize=1)
def _batch(n, n_cu):
    """carry_batch (its coverage condition is asserted inside, before anything is launched) and the row sets of the checks."""
    x, control, kinds = lc.carry_batch(n, n_cu)
    x.setflags(write=False)
    control.setflags(write=False)
    rows = {k: [i for i, kind in enumerate(kinds) if kind == k] for k in lc.CARRY_KINDS}
    plain, tone = lc.carry_sample_rows(kinds, n_cu)
    return x, control, rows, plain, tone


@functools.lru_cache(maxsize=None)
def _oracle(n, n_cu, normalize):
    x, _, _, plain, tone = _batch(n, n_cu)
    return lc.oracle_mel(x[plain + tone], n, normalize)


def _logmel(x, n, normalize, dev):
    t = x if isinstance(x, torch.Tensor) else torch.tensor(x, device=dev)
    return (ops.logmel(t, normalize) if n == 16000 else ops.logmel_frames(t, n, normalize)).cpu().numpy()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# n = 32000 (T = 63) with the normalisation only: its second run adds a fifth of a gigabyte of transfers and no other code path
@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("n,normalize", [(16000, True), (16000, False), (4000, True), (4000, False), (32000, True)])
def test_rows_do_not_depend_on_their_predecessor(dev, n_cu, math, n, normalize):
    """Enters the second (and third) iteration of the clip loop of logmel_kernel<., 4, 32> / <., 4, 64> (f32, auto), of
    logmel64_kernel<., false> (f64) and of logmel64_kernel<., true> (auto: the tone rows are marked), 32-frame tile at n = 16000 and
    64-frame tile at T = 8 and 63: B = 6 CUs + 41 is more than twice the widest grid."""
    x, control, rows, plain, tone = _batch(n, n_cu)
    B = len(x)
    assert B > 2 * 3 * n_cu
    ops.set_logmel_math(math)
    try:
        xd = torch.tensor(x, device=dev)
        out = _logmel(xd, n, normalize, dev)
        ctl = _logmel(control, n, normalize, dev)
        small = np.concatenate([_logmel(xd[c:c + n_cu], n, normalize, dev) for c in range(0, B, n_cu)])     # 8 waves, one clip each
        if math == "auto":
            ops.set_logmel_math("f32")
            f32 = _logmel(xd, n, normalize, dev)
    finally:
        ops.set_logmel_math("auto")
    assert out.shape == (B, 1, 80, 1 + n // 512)
    # (a) special rows all-NaN, every other row the control batch's bits; a silent row is 0 / 0 with the normalisation and the all-zero
    #     image without it (its control row holds a noisy clip, so it is checked on its own)
    if normalize:
        lc.check_rows(out, rows["special"] + rows["silent"], ctl)
    else:
        keep = np.setdiff1d(np.arange(B), rows["silent"])
        lc.check_rows(out[keep], np.flatnonzero(np.isin(keep, rows["special"])), ctl[keep])
        assert not out[rows["silent"]].any(), "a silent row is not the all-zero image"
    # (b) the looping form == one clip per workgroup, every row (NaN rows by position)
    bad = [i for i in range(B) if not _same(out[i], small[i])]
    assert not bad, f"{len(bad)} rows differ from launches of at most {n_cu} clips, first {bad[:8]}"
    # (c) rows that directly follow a special, a silent and a tone row in their workgroup, for every grid, against the oracle
    ref = _oracle(n, n_cu, normalize)
    err = np.abs(out[plain + tone] - ref).max(axis=(1, 2, 3))
    print(f"{math} normalize={normalize} n={n} B={B}: max|err| noisy/loud {err[:len(plain)].max():.3e}, tone {err[len(plain):].max():.3e}")
    assert err[:len(plain)].max() <= MEL_TOL, err
    if math != "f32":                     # noise-free rows: the auto and f64 modes only, as everywhere else
        assert err[len(plain):].max() <= MEL_TOL, err
    # (d) auto mode leaves a noisy row to the float kernel whatever ran before it in its workgroup: nothing downstream of a marked clip
    #     gets marked
    if math == "auto":
        bad = [i for i in rows["noisy"] if not np.array_equal(out[i], f32[i])]
        assert not bad, f"{len(bad)} noisy rows differ between auto and f32, first {bad[:8]}"
        assert any(not np.array_equal(out[i], f32[i]) for i in rows["tone"]), "no tone row was redone in float64: nothing was marked"


@pytest.mark.parametrize("math", MATHS)
def test_short_rows_in_a_looping_batch(dev, n_cu, math):
    """test_short_rows_do_not_read_their_padding's layout at B = 6 CUs + 41: rows of 9000 valid samples as views into a wider buffer
    full of NaN, so that behind every row's end lies NaN, not the zeros the kernel pads with -- and now the prefetch chain crosses clip
    ends INSIDE a workgroup (the last frame of a clip fetches the first of clip + grid through rs_next), in logmel_kernel<., 4, 32>
    (n = 16000) and <., 4, 64> (n = 24000, T = 47).  Row stride 16000 (taken as it is), then 16001 from an odd offset (copied)."""
    valid, B = 9000, lc.carry_rows(n_cu)
    assert B > 2 * 3 * n_cu
    rows = np.stack([lc.noisy(50 + k, valid) for k in range(16)])[np.arange(B) % 16] * (1.0 - 0.01 * (np.arange(B) // 16))[:, None]
    rows = rows.astype(np.float32)
    rows[1::3] = lc.tones(16000)[np.arange(len(rows[1::3])) % 5, :valid]
    packed = torch.from_numpy(rows).to(dev)
    wide = torch.full((B, 16000), float("nan"), device=dev)
    wide[:, :valid] = packed
    odd = torch.full((B * 16001 + 1,), float("nan"), device=dev)[1:].view(B, 16001)
    odd[:, :valid] = packed
    ops.set_logmel_math(math)
    try:
        for n in (16000, 24000):
            want = _logmel(packed, n, True, dev)
            assert np.isfinite(want).all()
            assert np.array_equal(_logmel(wide[:, :valid], n, True, dev), want), n
            assert np.array_equal(_logmel(odd[:, :valid], n, True, dev), want), n
            small = np.concatenate([_logmel(packed[c:c + n_cu], n, True, dev) for c in range(0, B, n_cu)])
            assert np.array_equal(small, want), n
    finally:
        ops.set_logmel_math("auto")
    assert torch.isnan(wide[:, valid:]).all() and torch.isnan(odd[:, valid:]).all()


def _cfg(n):
    return type(f"AudioConfig{n}", (AudioConfig,), {"DURATION": n / 16000.0})


@pytest.mark.parametrize("math", MATHS)
def test_streaming_ring_form_beyond_the_resident_grid(dev, n_cu, math):
    """The ring instances: one StreamingDetector at 0.25 s windows (n = 4000, T = 8, hop 400) with 2 x 2 x CUs + 41 microphones, more
    than twice the grid of logmel_kernel<true, 4, 64> (2 per CU) and four times logmel64_kernel<true, ., 64>'s (1 per CU), so every
    workgroup walks several microphones' rings.  The microphones follow carry_kinds; a special microphone gets one NaN sample in hop 2.
    14 hops: the ring wraps (10 hops) and the NaN leaves the window again.  Every step's logits and probabilities equal, bit for bit,
    those of three detectors of 24 microphones (8 waves, one ring per workgroup) fed the same hops: the first rows, the rows around the
    grid's end, and the last rows (third iteration)."""
    n, hop, n_hops, bad_hop = 4000, 400, 14, 2
    M = 2 * 2 * n_cu + 41
    kinds = lc.carry_kinds(M, n_cu, grids_per_cu=(1, 2))         # asserted before anything is launched
    m = pkg.SimpleWakewordModel(audio_config=_cfg(n))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in pkg.synth.make_state_dict("simple", seed=1234).items()})
    m = m.to(dev).eval()
    L = n_hops * hop
    noisy, tones = np.stack([lc.noisy(600 + k, L) for k in range(16)]), lc.tones(L)
    audio = np.zeros((M, L), np.float32)
    for i, kind in enumerate(kinds):
        if kind in ("noisy", "special"):
            audio[i] = noisy[i % 16] * np.float32(1.0 - 0.3 * i / M)
        elif kind == "tone":
            audio[i] = tones[i % 3]                              # the three tones that sound in every window
        elif kind == "loud":
            audio[i] = lc.scaled(noisy[i % 16], 15)
        if kind == "special":
            audio[i, bad_hop * hop + 123 + i % 200] = np.nan
    special = np.array([k == "special" for k in kinds])
    silent = np.array([k == "silent" for k in kinds])
    last_inside = bad_hop + n // hop - 1
    assert last_inside < n_hops - 1
    g = 2 * n_cu
    groups = [np.arange(0, 24), np.arange(g - 12, g + 12), np.arange(M - 24, M)]
    assert all({kinds[i] for i in grp} == set(lc.CARRY_KINDS) for grp in groups)
    ops.set_logmel_math(math)
    try:
        det = pkg.StreamingDetector(m, n_mics=M, hop_samples=hop, threshold=0.0)
        ctl = [pkg.StreamingDetector(m, n_mics=len(grp), hop_samples=hop, threshold=0.0) for grp in groups]
        for k in range(n_hops):
            h = audio[:, k * hop:(k + 1) * hop]
            det.step(torch.from_numpy(h).to(dev))
            for c, grp in zip(ctl, groups):
                c.step(torch.from_numpy(h[grp]).to(dev))
            fired = det.detections().cpu().numpy()                # waits for the detector's stream
            logits, prob = det.logits.cpu().numpy(), det.prob.cpu().numpy()
            for c, grp in zip(ctl, groups):
                c.stream.synchronize()
                assert _same(logits[grp], c.logits.cpu().numpy()) and _same(prob[grp], c.prob.cpu().numpy()), (k, grp[0])
            nan_now = silent | (special & (bad_hop <= k <= last_inside))
            assert np.isnan(prob[nan_now]).all() and np.isnan(logits[nan_now]).all() and not fired[nan_now].any(), k
            assert np.isfinite(prob[~nan_now]).all() and np.isfinite(logits[~nan_now]).all() and fired[~nan_now].all(), k
        det.close()
        for c in ctl:
            c.close()
    finally:
        ops.set_logmel_math("auto")
