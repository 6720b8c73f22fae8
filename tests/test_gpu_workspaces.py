"""Workspace contracts of the C ABI: poison, stale and guard-band tests for every entry point that takes a caller-owned buffer.

The header promises a size per workspace and nothing about its content.  Each entry below is called through `_native.lib` on
harness-owned buffers (tests/ws_harness.py) and must show, by bit equality:
  (1) content independence   the same output bytes on a 0x00-filled and on a 0xFF-filled workspace, equal to the ordinary wrapper's
  (2) stale independence     the larger shape, then the smaller one on the same workspace with no refill: the smaller one's bytes of (1)
  (3) bounds                 the guards of the workspace (EXACTLY the queried size) and of every output are intact after each call
0xFF is a quiet NaN as a float and -1 as an integer, so what matters before the first run is where a workspace holds indices or
counts, and who writes them first.  Read from the sources (csrc/), per entry:

  ww_cnn_pool_f32, n_conv 3 (launch_cnn_pool)          [mid: relu(conv2), n x 80 x 64 x 32 floats (f16x3d: f16 halves)] [apow2: n floats, 2^a2
      per clip, f16x3 only].  Floats only.  conv2's kernel writes every mid row of clips < n and apow2[clip] before conv3's kernel (next
      launch on the stream) reads them; the producer / consumer handshakes of the persistent kernels live in LDS.  n_conv 2: no scratch.
  ww_cnn_pool_wide_f32 (launch_cnn_pool_wide)          [partial: n K x C floats, one pooled row per column tile] [mid, apow2 of the n K
      virtual clips, n_conv 3].  Floats only.  The conv kernels write partial[tile] for every tile; pool_tiles_kernel reads exactly
      n K C of them.  A tile's halo columns are read from the mel image, not from scratch.
  ww_model_forward_f32 / ww_forward_pcm_f32 (carve)    [logmel n x 80 x 32] [pooled n x 128] [scratch as ww_cnn_pool_f32].  Floats, except
      that under log-mel math `auto` the float32 kernel leaves a mark and a frame mask in the first words of a marked clip's log-mel
      image for the float64 kernel: written by the float32 kernel for EVERY clip (dB or mark) before the float64 launch reads them.
      ww_model_forward_f32 leaves the logmel region alone.  pooled: conv stack writes n x C, the head reads n x C.
  ww_forward_pcm_frames_f32 / ww_forward_windows_f32   the same three regions with T = 1 + N / 512 columns and the wide scratch.
  ww_train_forward_f32 + ww_train_backward_f32 (carve_train)   floats: mid2, mid3, dz2, pooled, gates, masks, hd, lstm_packed, the packed
      conv operands, dhd / dg / dpooled / gp, the gradient partials [256 groups]; bit images (not indices): maskbits, bits1; wpk: the packed
      image, zeroed on the stream by the forward itself before pack_conv_h_dev writes it (its range[2] entry takes an atomic max); dgh:
      packed data-gradient operands, wmax [4] (zeroed on the stream by each launcher before its atomic max), gpmax [n], dzs [n] written
      by launch_gp_max / the conv3 data gradient before their readers.  No region holds an index, a count or a flag that the
      library does not write first; the arithmetic a workspace was written under is kept on the HOST, keyed by the pointer.
  ww_augment_n_f32, _bg_, _rir_ (launch_augment)       [records: n AugDev -- shifts, crops, frame counts: INDICES AND COUNTS] [buf_a] [buf_b]
      [spec] [y] floats, then [BgDev n] [RirDev n] slots (offsets, lengths: indices).  Every record is copied in from pinned memory on
      the stream (stage_to_device) before the first kernel; roll_kernel writes buf_a rows of clips < n first, each later stage reads
      what the stage before it wrote, up to the lengths in the records.
  ww_augment_records_n_f32, _bg_records_, _rir_records_   the same float regions; the records come from records_dev, written by the
      CALLER (here: into the workspace's own records region for the plain form, a buffer of their own for bg / rir), so only the bytes
      behind the records region are poisoned.
  ww_mix_background_f32, ww_reverb_f32, ww_rir_spectra_f32   [n records: offsets, lengths, taps -- indices], nothing else: staged in by
      the library before the one kernel that reads n of them.
  ww_events_sweep_f32                                  [s: n_windows float64 smoothed scores]: smooth_kernel writes s[i] for every window
      below min(offsets[n_segs], n_windows), event_sweep_kernel reads inside the same bound.
  ww_bank_gather_f32                                   [n_items ww_bank_item: offsets, starts, rows -- indices], staged in by the library.
  ww_bank_audit_f32                                    [hop_prefix: n + 1 int64 -- INDICES, built on the host and staged in by the library]
      [recs: one record per hop block]: bank_hops_kernel writes recs[g] for every g < hop_prefix[n], bank_entry_kernel reads those.
  ww_grad_norm_f32                                     [partial: one float64 per block]: grad_norm_kernel writes every partial[block],
      grad_norm_finish_kernel reads exactly `blocks` of them.
No read of an index or count that nothing wrote was found, so no kernel is changed.  Buffers the caller must initialise
(ww_events_step_f32's state, the ww_clip_metrics record) get property (3), and ww_clip_metrics_init must not care what the record held.

Teeth, on harness-owned buffers only: a byte written with torch next to either end of a workspace that a real call has just used is
seen; an output backed one element late by the workspace fails the bounds; and for the conv stack and the train step the workspace
interior differs from its fill after the call (the call really used the buffer it was handed, so (1) cannot pass vacuously)."""
import ctypes as C

import numpy as np
import pytest
import torch

import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import ops
from ws_harness import FILLS, Case, Guarded, as_bytes, check_content, check_stale, fresh, run

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
L = nat.lib
ARCH = {2: "simple", 3: "full"}
_CACHE = {}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _packed(n_conv):
    return _cached(("packed", n_conv), lambda: torch.from_numpy(ops.pack_state_dict(pkg.synth.make_state_dict(ARCH[n_conv], seed=1234))).to(DEV))


def _mel(n, width, seed=7):
    """[n, 1, 80, width] in the log-mel range, fixed by the seed; clip c is the same for every n."""
    def make():
        r = np.random.default_rng(seed)
        return torch.from_numpy((r.standard_normal((17, 1, 80, 63)) * 15 - 35).clip(-80, 0).astype(np.float32))
    full = _cached(("mel", seed), make)
    return full[:n, :, :, :width].contiguous().to(DEV)


def _pcm(n, samples, seed=11):
    """[n, samples] float32 on the device, rows 16-byte aligned with a stride that is a multiple of 4.  Clip 0 is a pure tone (no noise
    floor: log-mel math `auto` marks it for the float64 kernel), the rest tone + noise."""
    def make():
        r = np.random.default_rng(seed)
        t = np.arange(32000) / 16000.0
        x = np.stack([0.4 * np.sin(2 * np.pi * (180.0 + 37.0 * c) * t) + (0.0 if c == 0 else 0.05) * r.standard_normal(32000) for c in range(17)])
        return torch.from_numpy(x.astype(np.float32))
    full = _cached(("pcm", seed), make)
    buf = torch.zeros((n, (samples + 3) // 4 * 4), dtype=torch.float32, device=DEV)
    buf[:, :samples] = full[:n, :samples].to(DEV)
    return buf[:, :samples]


def _out(shape, dtype=torch.float32):
    return Guarded.for_output(shape, dtype, device=DEV)


@pytest.fixture
def conv_math(request):
    ops.set_conv_math(request.param)
    yield request.param
    ops.set_conv_math("f16x3")


@pytest.fixture
def logmel_math(request):
    ops.set_logmel_math(request.param)
    yield request.param
    ops.set_logmel_math("auto")


def _both(large, small):
    """Properties (1) and (3) for `small`, then (2) after `large` (skipped where they are one shape)."""
    expected, ws = check_content(small, DEV)
    if large.name != small.name:
        check_stale(large, small, expected, DEV)
    return expected, ws


# ---- ww_cnn_pool_f32, n_conv 3 -------------------------------------------------------------------------------------------------------
def _cnn_pool_case(n, width):
    x, packed = _mel(n, width), _packed(3)

    def call(ws, nbytes, outs):
        nat.check(L.ww_cnn_pool_f32(x.data_ptr(), n, width, packed.data_ptr(), 3, ws, outs["pooled"].ptr, _stream()))
    return Case(f"ww_cnn_pool_f32(n={n}, width={width}, n_conv=3)", lambda: L.ww_cnn_scratch_bytes(n, 3), call,
                lambda: {"pooled": _out((n, 128))}, wrapper=lambda: {"pooled": ops.cnn_pool(x, packed, 3)})


@pytest.mark.parametrize("width", [8, 31, 32])
@pytest.mark.parametrize("n", [1, 5, 17])
def test_cnn_pool_scratch(n, width):
    _, ws = _both(_cnn_pool_case(17, 32), _cnn_pool_case(n, width))
    assert ws.touched(), "the conv stack left the scratch it was handed untouched: the poison run proves nothing"


# ---- ww_cnn_pool_wide_f32 ------------------------------------------------------------------------------------------------------------
def _cnn_wide_case(n, width, n_conv):
    x, packed = _mel(n, width), _packed(n_conv)

    def call(ws, nbytes, outs):
        nat.check(L.ww_cnn_pool_wide_f32(x.data_ptr(), n, width, packed.data_ptr(), n_conv, ws, outs["pooled"].ptr, _stream()))
    return Case(f"ww_cnn_pool_wide_f32(n={n}, width={width}, n_conv={n_conv})", lambda: L.ww_cnn_wide_scratch_bytes(n, width, n_conv), call,
                lambda: {"pooled": _out((n, ops.c_last(n_conv)))}, wrapper=lambda: {"pooled": ops.cnn_pool_wide(x, packed, n_conv)})


@pytest.mark.parametrize("conv_math", ["f16x3", "f32"], indirect=True)
@pytest.mark.parametrize("n_conv", [2, 3])
@pytest.mark.parametrize("width", [33, 47, 63])
@pytest.mark.parametrize("n", [1, 5])
def test_cnn_wide_scratch(n, width, n_conv, conv_math):
    _, ws = _both(_cnn_wide_case(5, 63, n_conv), _cnn_wide_case(n, width, n_conv))
    assert ws.touched()


# ---- ww_model_forward_f32 ------------------------------------------------------------------------------------------------------------
def _model_forward_case(n, width, n_conv):
    x, packed = _mel(n, width), _packed(n_conv)

    def call(ws, nbytes, outs):
        nat.check(L.ww_model_forward_f32(x.data_ptr(), n, width, packed.data_ptr(), n_conv, ws, outs["logits"].ptr, _stream()))
    return Case(f"ww_model_forward_f32(n={n}, width={width}, n_conv={n_conv})", lambda: L.ww_workspace_bytes(n, n_conv), call,
                lambda: {"logits": _out((n, 2))}, wrapper=lambda: {"logits": ops.cnn_lstm_forward(x, packed, n_conv)})


@pytest.mark.parametrize("n_conv", [2, 3])
@pytest.mark.parametrize("width", [8, 32])
@pytest.mark.parametrize("n", [1, 5, 17])
def test_model_forward_workspace(n, width, n_conv):
    _both(_model_forward_case(17, 32, n_conv), _model_forward_case(n, width, n_conv))


# ---- ww_forward_pcm_f32 --------------------------------------------------------------------------------------------------------------
def _forward_pcm_case(n, clip_len, n_conv):
    pcm, packed = _pcm(n, clip_len), _packed(n_conv)

    def call(ws, nbytes, outs):
        nat.check(L.ww_forward_pcm_f32(pcm.data_ptr(), n, pcm.stride(0) if n > 1 else clip_len, clip_len, 1, packed.data_ptr(), n_conv, ws,
                                       outs["logits"].ptr, _stream()))
    return Case(f"ww_forward_pcm_f32(n={n}, clip_len={clip_len}, n_conv={n_conv})", lambda: L.ww_workspace_bytes(n, n_conv), call,
                lambda: {"logits": _out((n, 2))}, wrapper=lambda: {"logits": ops.forward_pcm(pcm, packed, n_conv, True)})


@pytest.mark.parametrize("logmel_math", ["auto", "f64"], indirect=True)
@pytest.mark.parametrize("n_conv", [2, 3])
@pytest.mark.parametrize("clip_len", [16000, 9000])
@pytest.mark.parametrize("n", [1, 5, 17])
def test_forward_pcm_workspace(n, clip_len, n_conv, logmel_math):
    _both(_forward_pcm_case(17, 16000, n_conv), _forward_pcm_case(n, clip_len, n_conv))


# ---- ww_forward_pcm_frames_f32 -------------------------------------------------------------------------------------------------------
def _forward_frames_case(n, n_samples, n_conv):
    pcm, packed = _pcm(n, n_samples), _packed(n_conv)

    def call(ws, nbytes, outs):
        nat.check(L.ww_forward_pcm_frames_f32(pcm.data_ptr(), n, pcm.stride(0) if n > 1 else n_samples, n_samples, n_samples, 1,
                                              packed.data_ptr(), n_conv, ws, outs["logits"].ptr, _stream()))
    return Case(f"ww_forward_pcm_frames_f32(n={n}, n_samples={n_samples}, n_conv={n_conv})",
                lambda: L.ww_workspace_frames_bytes(n, n_samples, n_conv), call, lambda: {"logits": _out((n, 2))},
                wrapper=lambda: {"logits": ops.forward_pcm_frames(pcm, packed, n_conv, n_samples, True)})


@pytest.mark.parametrize("n_conv", [2, 3])
@pytest.mark.parametrize("n_samples", [4000, 12345, 24000])
@pytest.mark.parametrize("n", [1, 5])
def test_forward_frames_workspace(n, n_samples, n_conv):
    _both(_forward_frames_case(5, 24000, n_conv), _forward_frames_case(n, n_samples, n_conv))


# ---- ww_forward_windows_f32 ----------------------------------------------------------------------------------------------------------
HOP = 160


def _forward_windows_case(n_windows, n_samples, n_conv, with_prob):
    packed = _packed(n_conv)
    signal = Guarded.holding(_pcm(1, (19 - 1) * HOP + 16000, seed=13)[0, :(n_windows - 1) * HOP + n_samples], align=16)

    def outs():
        o = {"logits": _out((n_windows, 2))}
        if with_prob:
            o["prob"] = _out((n_windows,))
        return o

    def call(ws, nbytes, o):
        nat.check(L.ww_forward_windows_f32(signal.ptr, n_windows, HOP, n_samples, 1, packed.data_ptr(), n_conv, ws, nbytes, o["logits"].ptr,
                                           o["prob"].ptr if with_prob else None, _stream()))

    def wrapper():                                          # the header: bit for bit the PCM entry points on the windows copied out as rows
        rows = signal.view().unfold(0, n_samples, HOP).contiguous()
        assert rows.shape == (n_windows, n_samples)
        if n_samples == 16000:
            return {"logits": ops.forward_pcm(rows, packed, n_conv, True)}
        return {"logits": ops.forward_pcm_frames(rows, packed, n_conv, n_samples, True)}
    return Case(f"ww_forward_windows_f32(n_windows={n_windows}, n_samples={n_samples}, n_conv={n_conv}, prob={with_prob})",
                lambda: L.ww_forward_windows_workspace_bytes(n_windows, n_samples, n_conv), call, outs, wrapper=wrapper,
                inputs={"signal": signal})


@pytest.mark.parametrize("with_prob", [False, True])
@pytest.mark.parametrize("n_conv", [2, 3])
@pytest.mark.parametrize("n_samples", [16000, 8000])
@pytest.mark.parametrize("n_windows", [1, 19])
def test_forward_windows_workspace(n_windows, n_samples, n_conv, with_prob):
    expected, _ = _both(_forward_windows_case(19, 16000, n_conv, with_prob), _forward_windows_case(n_windows, n_samples, n_conv, with_prob))
    if with_prob:                                           # p(wakeword) is a probability of the same logits
        z = expected["logits"].view(torch.float32).view(n_windows, 2).double()
        p = expected["prob"].view(torch.float32).double()
        assert torch.allclose(p, torch.softmax(z, 1)[:, 1], rtol=0, atol=1e-6)


# ---- ww_train_forward_f32 + ww_train_backward_f32 ------------------------------------------------------------------------------------
GRAD_KEYS = {2: ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias"),
             3: ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias")}
HEAD_KEYS = ("lstm.weight_ih_l0", "lstm.bias_ih_l0", "lstm.weight_ih_l1", "lstm.bias_ih_l1", "fc.weight", "fc.bias")


def _train_params(n_conv):
    def make():
        sd = pkg.synth.make_state_dict(ARCH[n_conv], seed=5)
        return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in sd.items()}
    return _cached(("train params", n_conv), make)


def _train_case(n, width, n_conv, math, p_drop):
    """The parameter and gradient plumbing of tests/test_gpu_train_stages.py (ops._train_keys / ops._train_params_struct) on guarded
    gradient buffers; the workspace is poisoned before the forward only (it must stay untouched until the backward)."""
    named = _train_params(n_conv)
    keys = ops._train_keys(n_conv)
    params = [named[k] for k in keys]
    x = _mel(n, width, seed=3)
    dlogits = _cached(("dlogits", n), lambda: torch.from_numpy((np.random.default_rng(n).standard_normal((n, 2)) / n).astype(np.float32)).to(DEV))
    seed, mode = 1234, ops.TRAIN_MATH[math]
    grad_keys = GRAD_KEYS[n_conv] + HEAD_KEYS

    def outs():
        o = {"logits": _out((n, 2))}
        o.update({k: _out(tuple(named[k].shape)) for k in grad_keys})
        return o

    def call(ws, nbytes, o):
        tp = ops._train_params_struct(params, n_conv)
        nat.check(L.ww_train_forward_f32(x.data_ptr(), n, width, C.byref(tp), p_drop, p_drop, seed, mode, ws, nbytes, o["logits"].ptr, _stream()))
        tg = nat.TrainGrads()
        for i in range(n_conv):
            tg.conv_weight[i], tg.conv_bias[i] = o[f"conv{i + 1}.weight"].ptr, o[f"conv{i + 1}.bias"].ptr
        tg.lstm_weight_ih[0], tg.lstm_bias[0] = o["lstm.weight_ih_l0"].ptr, o["lstm.bias_ih_l0"].ptr
        tg.lstm_weight_ih[1], tg.lstm_bias[1] = o["lstm.weight_ih_l1"].ptr, o["lstm.bias_ih_l1"].ptr
        tg.fc_weight, tg.fc_bias = o["fc.weight"].ptr, o["fc.bias"].ptr
        nat.check(L.ww_train_backward_f32(x.data_ptr(), n, width, C.byref(tp), dlogits.data_ptr(), mode, ws, nbytes, C.byref(tg), _stream()))

    def wrapper():
        before = ops.get_train_math()
        ops.set_train_math(math)
        try:
            leaves = {k: named[k].clone().requires_grad_(True) for k in keys}
            logits = ops.train_forward(x, leaves, n_conv, p_drop, p_drop, seed)
            logits.backward(dlogits)
            got = {k: leaves[k].grad for k in grad_keys}
            got["logits"] = logits.detach()
            return got
        finally:
            ops.set_train_math(before)
    return Case(f"ww_train step(n={n}, width={width}, n_conv={n_conv}, {math}, dropout={p_drop})",
                lambda: L.ww_train_workspace_bytes(n, n_conv, mode), call, outs, wrapper=wrapper)


@pytest.mark.parametrize("p_drop", [0.0, 0.3])
@pytest.mark.parametrize("math", ["f32", "f16x3"])
@pytest.mark.parametrize("n_conv", [2, 3])
@pytest.mark.parametrize("width", [8, 32])
@pytest.mark.parametrize("n", [1, 5, 17])
def test_train_step_workspace(n, width, n_conv, math, p_drop):
    _, ws = _both(_train_case(17, 32, n_conv, math, p_drop), _train_case(n, width, n_conv, math, p_drop))
    assert ws.touched(), "the train step left the workspace it was handed untouched: the poison run proves nothing"


# ---- augmentation --------------------------------------------------------------------------------------------------------------------
def _plans(B, N):
    """A mixed batch: clip 0 has every transform on; then shift only, pitch only, stretch only, noise only."""
    rate = 0.9
    over = int(np.rint(N / rate)) - N
    every = {"shift": 1234, "n_steps": 2.0, "rate": rate, "crop": min(100, over), "sigma": 0.005, "seed": 99}
    single = [{"shift": -777}, {"n_steps": -3.0}, {"rate": 1.25}, {"sigma": 0.01, "seed": 5}]
    return ([every] + single)[:B]


def _bg_bank():
    def make():
        r = np.random.default_rng(21)
        lengths = [3000, 9000, 20000]
        return pkg.BackgroundNoiseBank.from_buffer(torch.from_numpy((0.1 * r.standard_normal(sum(lengths))).astype(np.float32)).to(DEV), lengths)
    return _cached("bg bank", make)


RIR_TAPS = (300, 2000, 1, 4097, 777)


def _rir_taps():
    """Impulse responses whose direct path is their first and largest tap: the bank's trimming rule keeps every tap."""
    def make():
        r = np.random.default_rng(23)
        hs = []
        for k in RIR_TAPS:
            h = (0.2 * r.standard_normal(k) * np.exp(-np.arange(k) / (0.2 * k + 1))).astype(np.float32)
            h[0] = 1.0
            hs.append(h)
        return hs
    return _cached("rir taps", make)


def _rir_bank():
    def make():
        bank = pkg.ImpulseResponseBank.from_taps(_rir_taps(), device=DEV)
        assert list(bank.lengths) == list(RIR_TAPS) and not bank.dpos.any()
        return bank
    return _cached("rir bank", make)


def _with_bg(plans):
    out = []
    for i, p in enumerate(plans):
        q = dict(p)
        if i != 3:                                          # one clip of a full batch without background
            q.update(bg_file=i % 3, bg_start=17 * i + 1, snr_db=10.0 - 3.0 * i)
        out.append(q)
    return out


def _with_rir(plans):
    out = []
    for i, p in enumerate(plans):
        q = dict(p)
        if i != 2:
            q["rir"] = (i + 1) % len(RIR_TAPS)
        out.append(q)
    return out


def _augment_case(kind, B, N, records):
    """kind: "n" (ww_augment_n_f32), "bg", "rir"; records: the two-call form (prepare on the host, the launch reads records_dev)."""
    pcm = _pcm(B, N, seed=17)
    stride = pcm.stride(0) if B > 1 else N
    plans = _plans(B, N)
    bank, rirs = _bg_bank(), _rir_bank()
    if kind != "n":
        plans = _with_bg(plans)
    if kind == "rir":
        plans = _with_rir(plans)
    arr = ops._plans_array(plans, B)
    bg = ops._bg_array(plans, bank, B) if kind != "n" else None
    rir = ops._rir_array(plans, rirs, B) if kind == "rir" else None
    bank_ptr, bank_len = bank.data.data_ptr(), bank.data.numel()
    spectra_ptr, n_rirs = rirs.spectra.data_ptr(), rirs.n_rirs
    size = {"n": lambda: L.ww_augment_n_workspace_bytes(B, N), "bg": lambda: L.ww_augment_bg_workspace_bytes(B, N),
            "rir": lambda: L.ww_augment_rir_workspace_bytes(B, N)}[kind]
    lay = nat.AugmentLayout()
    nat.check(L.ww_augment_workspace_layout(B, N, C.byref(lay)))
    name = f"ww_augment_{kind}{'_records' if records else ''}_f32(B={B}, N={N})"
    make_outs = lambda: {"out": _out((B, N))}                                                      # noqa: E731
    wrapper = lambda: {"out": ops.augment(pcm, plans, bank=bank if kind != "n" else None, rirs=rirs if kind == "rir" else None)}   # noqa: E731
    if not records:
        def call(ws, nbytes, o):
            if kind == "n":
                nat.check(L.ww_augment_n_f32(pcm.data_ptr(), B, stride, N, arr, o["out"].ptr, N, ws, _stream()))
            elif kind == "bg":
                nat.check(L.ww_augment_bg_f32(pcm.data_ptr(), B, stride, N, arr, bg, bank_ptr, bank_len, o["out"].ptr, N, ws, _stream()))
            else:
                nat.check(L.ww_augment_rir_f32(pcm.data_ptr(), B, stride, N, arr, bg, bank_ptr, bank_len, rir, spectra_ptr, n_rirs, o["out"].ptr, N,
                                               ws, _stream()))
        return Case(name, size, call, make_outs, wrapper=wrapper)
    per_clip = {"n": L.ww_augment_record_bytes, "bg": L.ww_augment_bg_record_bytes, "rir": L.ww_augment_rir_record_bytes}[kind]()
    host = np.zeros(B * per_clip, np.uint8)
    if kind == "n":
        nat.check(L.ww_augment_plans_prepare_n(arr, B, N, host.ctypes.data))
    elif kind == "bg":
        nat.check(L.ww_augment_bg_prepare(arr, bg, B, N, bank_len, host.ctypes.data))
    else:
        nat.check(L.ww_augment_rir_prepare(arr, bg, rir, B, N, bank_len, n_rirs, host.ctypes.data))
    rec_dev = torch.from_numpy(host).to(DEV)
    assert lay.records == 0 and lay.buf_a >= B * lay.record_bytes

    def prepare(ws):                                        # the plain form keeps its records in the workspace's own records region
        if kind == "n":
            ws.interior[:host.size].copy_(rec_dev)

    def call(ws, nbytes, o):
        rp = ws + lay.records if kind == "n" else rec_dev.data_ptr()
        if kind == "n":
            nat.check(L.ww_augment_records_n_f32(pcm.data_ptr(), B, stride, N, rp, o["out"].ptr, N, ws, _stream()))
        elif kind == "bg":
            nat.check(L.ww_augment_bg_records_f32(pcm.data_ptr(), B, stride, N, rp, bank_ptr, bank_len, o["out"].ptr, N, ws, _stream()))
        else:
            nat.check(L.ww_augment_rir_records_f32(pcm.data_ptr(), B, stride, N, rp, bank_ptr, bank_len, spectra_ptr, n_rirs, o["out"].ptr, N, ws,
                                                   _stream()))
    return Case(name, size, call, make_outs, wrapper=wrapper, poison_from=lay.buf_a, prepare=prepare)


@pytest.mark.parametrize("records", [False, True])
@pytest.mark.parametrize("N", [4000, 16000])
@pytest.mark.parametrize("B", [1, 5])
def test_augment_n_workspace(B, N, records):
    _, ws = _both(_augment_case("n", 5, 16000, records), _augment_case("n", B, N, records))
    assert ws.touched(start=_augment_case("n", B, N, records).poison_from)


@pytest.mark.parametrize("records", [False, True])
@pytest.mark.parametrize("kind", ["bg", "rir"])
@pytest.mark.parametrize("N", [4000, 16000])
@pytest.mark.parametrize("B", [1, 5])
def test_augment_bg_rir_workspace(B, N, kind, records):
    _both(_augment_case(kind, 5, 16000, records), _augment_case(kind, B, N, records))


def _mix_case(B, N):
    pcm, bank = _pcm(B, N, seed=17), _bg_bank()
    files, starts, snr = [i % 3 if i != 3 else -1 for i in range(B)], [17 * i + 1 for i in range(B)], [10.0 - 3.0 * i for i in range(B)]
    bg = ops._bg_array([{} if f < 0 else {"bg_file": f, "bg_start": s, "snr_db": d} for f, s, d in zip(files, starts, snr)], bank, B)

    def call(ws, nbytes, o):
        nat.check(L.ww_mix_background_f32(pcm.data_ptr(), B, pcm.stride(0) if B > 1 else N, N, bg, bank.data.data_ptr(), bank.data.numel(),
                                          o["out"].ptr, N, ws, _stream()))
    return Case(f"ww_mix_background_f32(B={B}, N={N})", lambda: L.ww_mix_background_workspace_bytes(B), call, lambda: {"out": _out((B, N))},
                wrapper=lambda: {"out": ops.mix_background(pcm, bank, files, starts, snr)})


def _reverb_case(B, N):
    pcm, rirs = _pcm(B, N, seed=17), _rir_bank()
    index = [(i + 1) % len(RIR_TAPS) if i != 2 else -1 for i in range(B)]
    rir = ops._rir_array([{} if r < 0 else {"rir": r} for r in index], rirs, B)

    def call(ws, nbytes, o):
        nat.check(L.ww_reverb_f32(pcm.data_ptr(), B, pcm.stride(0) if B > 1 else N, N, rir, rirs.spectra.data_ptr(), rirs.n_rirs, o["out"].ptr, N,
                                  ws, _stream()))
    return Case(f"ww_reverb_f32(B={B}, N={N})", lambda: L.ww_reverb_workspace_bytes(B), call, lambda: {"out": _out((B, N))},
                wrapper=lambda: {"out": ops.reverb(pcm, rirs, index)})


def _rir_spectra_case(n_rirs):
    taps = _rir_taps()[:n_rirs]
    buf = torch.from_numpy(np.concatenate(taps)).to(DEV)
    lengths = np.array([t.size for t in taps], np.int32)
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)

    def call(ws, nbytes, o):
        nat.check(L.ww_rir_spectra_f32(buf.data_ptr(), buf.numel(), offsets.ctypes.data, lengths.ctypes.data, n_rirs, o["spectra"].ptr, ws, _stream()))
    return Case(f"ww_rir_spectra_f32(n_rirs={n_rirs})", lambda: L.ww_rir_spectra_workspace_bytes(n_rirs), call,
                lambda: {"spectra": _out((n_rirs, nat.RIR_SPECTRUM_BINS, 2))},
                wrapper=lambda: {"spectra": pkg.ImpulseResponseBank.from_taps(taps, device=DEV).spectra})


@pytest.mark.parametrize("N", [4000, 20000])
@pytest.mark.parametrize("B", [1, 5])
def test_mix_background_workspace(B, N):
    _both(_mix_case(5, 20000), _mix_case(B, N))


@pytest.mark.parametrize("B", [1, 5])
def test_reverb_workspace(B):
    _both(_reverb_case(5, 4000), _reverb_case(B, 4000))


@pytest.mark.parametrize("n_rirs", [1, 5])
def test_rir_spectra_workspace(n_rirs):
    _both(_rir_spectra_case(5), _rir_spectra_case(n_rirs))


# ---- ww_events_sweep_f32 -------------------------------------------------------------------------------------------------------------
def _events_case(n_windows, n_thr, smooth):
    """3 segments (the middle one takes the odd window; with one window the outer two are empty), refractory 3 windows."""
    counts = [n_windows // 3, n_windows - 2 * (n_windows // 3), n_windows // 3]
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    r = np.random.default_rng(31)
    p = r.random(n_windows).astype(np.float32)
    p[::11] = np.nan                                        # a non-finite score counts as 0
    prob, seg_dev = torch.from_numpy(p).to(DEV), torch.from_numpy(seg).to(DEV)
    thr = np.linspace(0.3, 0.9, n_thr).astype(np.float32)
    thr_dev = torch.from_numpy(thr).to(DEV)
    R = 3

    def outs():
        o = {"counts": _out((3, n_thr), torch.int64)}
        if n_thr == 1:
            o["fired"] = _out((n_windows,), torch.uint8)
        return o

    def call(ws, nbytes, o):
        nat.check(L.ww_events_sweep_f32(prob.data_ptr(), seg_dev.data_ptr(), 3, n_windows, smooth, R, thr_dev.data_ptr(), n_thr, o["counts"].ptr,
                                        o["fired"].ptr if n_thr == 1 else None, ws, nbytes, _stream()))

    def wrapper():                                          # Scan's sweep: hop = 1 s, so files of `counts` seconds hold `counts` windows
        scan = pkg.Scan(prob, [c * 16000 for c in counts], ["a", "b", "c"], [], 16000, 16000, None, DEV)
        assert scan.window_offsets.tolist() == seg.tolist()
        c, f = scan._sweep(thr, smooth, float(R), n_thr == 1)
        got = {"counts": torch.from_numpy(c)}
        if n_thr == 1:
            got["fired"] = torch.from_numpy(f)
        return got
    return Case(f"ww_events_sweep_f32(n_windows={n_windows}, n_thr={n_thr}, smooth={smooth})", lambda: L.ww_events_workspace_bytes(n_windows),
                call, outs, wrapper=wrapper, align=16)


@pytest.mark.parametrize("smooth", [1, 8])
@pytest.mark.parametrize("n_thr", [1, 7])
@pytest.mark.parametrize("n_windows", [1, 257, 5000])
def test_events_sweep_workspace(n_windows, n_thr, smooth):
    expected, _ = _both(_events_case(5000, n_thr, smooth), _events_case(n_windows, n_thr, smooth))
    assert int(expected["counts"].view(torch.int64).sum()) > 0 or n_windows == 1


# ---- ww_bank_gather_f32 / ww_bank_audit_f32 ------------------------------------------------------------------------------------------
def _proc(n):
    from wakeword_jupyterlab_amd.config import AudioConfig
    return pkg.AudioProcessor(type(f"AudioConfig{n}", (AudioConfig,), {"DURATION": n / 16000.0}), device=DEV)


GATHER_LENGTHS = (0, 100, 4000, 7000, 12001)
GATHER_N = 4000


def _gather_bank():
    def make():
        r = np.random.default_rng(41)
        b = pkg.ClipBank(_proc(GATHER_N))
        b.add_buffer(torch.from_numpy((0.3 * r.standard_normal(sum(GATHER_LENGTHS) + 5)).astype(np.float32)).to(DEV), list(GATHER_LENGTHS))
        return b
    return _cached("gather bank", make)


def _gather_case(n_items, norm):
    from wakeword_jupyterlab_amd.bank import ITEM_DTYPE, NORMS
    b, N = _gather_bank(), GATHER_N
    entries = np.array([(3 * i + 1) % len(GATHER_LENGTHS) for i in range(n_items)], np.int64)
    lengths = b.lengths[entries]
    starts = np.array([[0, -N, int(l), int(l) // 2, -N // 3, max(0, int(l) - N)][i % 6] for i, l in enumerate(lengths)], np.int64)
    rows = np.arange(n_items, dtype=np.int64)[::-1].copy()  # rows in another order than the items
    items = np.zeros(n_items, ITEM_DTYPE)
    items["offset"], items["length"], items["start"] = b._off[entries], lengths, starts
    items["peak"], items["row"], items["norm"] = b.peaks[entries], rows, NORMS[norm]
    data = b.segments[0]

    def call(ws, nbytes, o):
        nat.check(L.ww_bank_gather_f32(data.data_ptr(), data.numel(), items.ctypes.data, n_items, N, o["out"].ptr, n_items, N, ws, _stream()))

    def wrapper():
        out = torch.empty((n_items, N), device=DEV, dtype=torch.float32)
        b.gather(entries, starts, normalize=norm, out=out, rows=rows)
        return {"out": out}
    return Case(f"ww_bank_gather_f32(n_items={n_items}, norm={norm})", lambda: L.ww_bank_gather_workspace_bytes(n_items), call,
                lambda: {"out": _out((n_items, N))}, wrapper=wrapper)


@pytest.mark.parametrize("norm", [None, "entry", "window"])
@pytest.mark.parametrize("n_items", [1, 37])
def test_bank_gather_workspace(n_items, norm):
    _both(_gather_case(37, norm), _gather_case(n_items, norm))


AUDIT_LENGTHS = (0, 1, 511, 512, 5000, 70000)


def _audit_case(n_entries):
    from wakeword_jupyterlab_amd.audit import STATS_DTYPE, top_db_ratio
    lengths = list(AUDIT_LENGTHS[:n_entries])

    def make():
        r = np.random.default_rng(43)
        x = (0.3 * r.standard_normal(sum(AUDIT_LENGTHS))).astype(np.float32)
        x[600:700] = 0.0
        x[-30000:-20000] *= 1e-4                            # a quiet stretch inside the long entry
        x[1500] = 1.5                                       # clipped
        return torch.from_numpy(x).to(DEV)
    data = _cached("audit data", make)[:max(1, sum(lengths))]
    table = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    off = torch.from_numpy(table).to(DEV)
    clip_level, ratio = float(np.float32(0.999)), top_db_ratio(60.0)

    def call(ws, nbytes, o):
        nat.check(L.ww_bank_audit_f32(data.data_ptr(), data.numel(), off.data_ptr(), table.ctypes.data, n_entries, clip_level, ratio, o["stats"].ptr,
                                      ws, _stream()))

    def wrapper():
        b = pkg.ClipBank(_proc(4000))
        b.add_buffer(data, lengths)
        stats = b.audit(60.0, 0.999).stats
        assert stats.dtype == STATS_DTYPE
        return {"stats": torch.from_numpy(stats.view(np.uint8).copy())}
    return Case(f"ww_bank_audit_f32(lengths={lengths})", lambda: L.ww_bank_audit_workspace_bytes(data.numel(), n_entries), call,
                lambda: {"stats": _out((n_entries * 72,), torch.uint8)}, wrapper=wrapper)


@pytest.mark.parametrize("n_entries", [3, 6])
def test_bank_audit_workspace(n_entries):
    expected, _ = _both(_audit_case(6), _audit_case(n_entries))
    from wakeword_jupyterlab_amd.audit import STATS_DTYPE
    stats = expected["stats"].cpu().numpy().view(STATS_DTYPE)
    assert stats["peak"][0] == 0 and stats["hash"][0] == 0 and (stats["peak"][1:] > 0).all()


# ---- ww_grad_norm_f32 ----------------------------------------------------------------------------------------------------------------
def _grad_norm_case(n_tensors):
    from test_gpu_trainer import SIZES
    assert len(SIZES) == 16

    def make():
        r = np.random.default_rng(51)
        gs = [torch.from_numpy(r.standard_normal(s).astype(np.float32)).to(DEV) for s in SIZES[:15]]
        return gs + [gs[14]]                                # the last two entries share one gradient
    grads = _cached("grad norm tensors", make)[:n_tensors]
    tab = ops.adam_table(None, grads, None, None)
    max_norm = 1.0

    def call(ws, nbytes, o):
        nat.check(L.ww_grad_norm_f32(tab, n_tensors, max_norm, o["norm"].ptr, o["scale"].ptr, ws, _stream()))

    def wrapper():
        norm, scale = ops.grad_norm(grads, max_norm)
        return {"norm": norm, "scale": scale}
    return Case(f"ww_grad_norm_f32({n_tensors} tensors)", lambda: L.ww_grad_norm_workspace_bytes(tab, n_tensors), call,
                lambda: {"norm": _out((1,), torch.float64), "scale": _out((1,))}, wrapper=wrapper)


@pytest.mark.parametrize("n_tensors", [5, 16])
def test_grad_norm_workspace(n_tensors):
    expected, ws = _both(_grad_norm_case(16), _grad_norm_case(n_tensors))
    norm = float(expected["norm"].view(torch.float64)[0])
    assert np.isfinite(norm) and norm > 1.0 and 0.0 < float(expected["scale"].view(torch.float32)[0]) < 1.0
    assert ws.touched()


# ---- buffers the caller initialises: bounds only, and an init that does not care what the buffer held ---------------------------------
@pytest.mark.parametrize("n_mics,smooth", [(1, 1), (5, 8), (300, 3)])
def test_preinitialised_events_state_bounds(n_mics, smooth):
    nbytes = nat.check(L.ww_events_state_bytes(n_mics, smooth))
    state = Guarded(nbytes, 0x00, align=16, device=DEV)    # zeroed before the first hop, as the header requires
    fired = _out((n_mics,), torch.uint8)
    r = np.random.default_rng(61)
    total = 0
    for _ in range(2 * smooth + 3):
        prob = torch.from_numpy(r.random(n_mics).astype(np.float32)).to(DEV)
        nat.check(L.ww_events_step_f32(prob.data_ptr(), n_mics, smooth, 0.4, 2, state.ptr, fired.ptr, _stream()))
        torch.cuda.synchronize()
        assert state.intact() and fired.intact()
        f = fired.view()
        assert bool(((f == 0) | (f == 1)).all())
        total += int(f.sum())
    assert total > 0 and state.touched()
    assert int(state.view(torch.int64, (2 * n_mics,))[0]) == 2 * smooth + 3          # hops seen by microphone 0


def test_preinitialised_clip_metrics_init_ignores_content():
    nbytes = nat.check(L.ww_clip_metrics_bytes())
    r = np.random.default_rng(63)
    logits = torch.from_numpy(r.standard_normal((300, 2)).astype(np.float32)).to(DEV)
    labels = torch.from_numpy(r.integers(0, 2, 300)).to(DEV)
    thr = (C.c_float * 3)(0.3, 0.5, 0.8)
    records = []
    for fill in FILLS:
        state = Guarded(nbytes, fill, align=8, device=DEV)
        nat.check(L.ww_clip_metrics_init(state.ptr, thr, 3, _stream()))
        nat.check(L.ww_clip_metrics_update_f32(logits.data_ptr(), labels.data_ptr(), 300, state.ptr, _stream()))
        torch.cuda.synchronize()
        assert state.intact()
        records.append(state.bytes())
        nat.check(L.ww_clip_metrics_reset(state.ptr, _stream()))
        torch.cuda.synchronize()
        assert state.intact()
    assert torch.equal(records[0], records[1])
    rec = nat.ClipMetrics.from_buffer_copy(records[0].cpu().numpy().tobytes())
    assert rec.total == 300 and rec.batches == 1 and rec.n_thresholds == 3 and sum(rec.argmax[a][b] for a in (0, 1) for b in (0, 1)) == 300
    st = ops.new_clip_metrics(DEV, (0.3, 0.5, 0.8))         # the wrapper's record after the same update
    ops.clip_metrics_update(logits, labels, st)
    assert torch.equal(records[0], as_bytes(st.buffer))


# ---- teeth: each check can fail, shown on harness-owned buffers -----------------------------------------------------------------------
def test_teeth_guard_bytes_next_to_a_used_workspace_are_watched():
    case = _cnn_pool_case(5, 31)
    for where in (-1, None):                                # the byte before the interior, the byte at interior + nbytes
        ws = fresh(case, 0xFF, DEV)
        run(case, ws, DEV)                                  # a real call: clean
        index = ws.start - 1 if where == -1 else ws.start + ws.nbytes
        ws.raw[index] = 0
        assert not ws.intact()


def test_teeth_an_output_backed_one_element_late_fails_the_bounds():
    """The pooled features written through a pointer one float late: the last float lands in the guard, and `run` says so."""
    case = _cnn_pool_case(5, 31)
    late = Case(case.name + " [output one float late]", case.size_query,
                lambda ws, nbytes, outs: case.call(ws, nbytes, {"pooled": _Shifted(outs["pooled"], 4)}), case.make_outs)
    with pytest.raises(AssertionError, match="outside output 'pooled'"):
        run(late, fresh(late, 0x00, DEV), DEV)


class _Shifted:
    def __init__(self, g, by):
        self.ptr = g.ptr + by


def test_teeth_content_and_stale_checks_see_a_dependence():
    """Stand-in 'entries' on harness-owned buffers: one copies the first float of the workspace it is handed into its output, one
    leaves a pattern there.  (1) fails on the first; (2) fails on the first run after the second."""
    def reads(ws_ptr, nbytes, outs):
        assert small.ws.ptr == ws_ptr
        outs["y"].interior.zero_()
        outs["y"].interior[:4].copy_(small.ws.interior[:4])

    def writes(ws_ptr, nbytes, outs):
        outs["y"].interior.zero_()
        large.ws.interior[:4].fill_(0x3F)
    small = Case("stand-in reader", lambda: 256, reads, lambda: {"y": _out((4,))})
    large = Case("stand-in writer", lambda: 512, writes, lambda: {"y": _out((4,))})
    with pytest.raises(AssertionError, match="depend on the workspace's content"):
        check_content(small, DEV)
    expected = run(small, fresh(small, 0x00, DEV), DEV)
    assert not bool(expected["y"].any())
    with pytest.raises(AssertionError, match="stand-in reader after stand-in writer"):
        check_stale(large, small, expected, DEV)
    check_stale(small, small, expected, DEV)               # and passes where nothing was left behind
