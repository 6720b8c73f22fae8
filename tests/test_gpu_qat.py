"""Quantisation-aware training on the GPU (csrc/ww_quant.hip): the clipped quantiser, the clip search and the
straight-through estimator against the numpy restatement of their rule (tests/qat_ref.py), WeightQuant(clip="mse"), and a QAT step of
WakewordTrainer against its parts.

Tolerances: none on scale, q, deq, sat, bad, clip and the masked gradients -- every step of the rule is one correctly rounded float32
operation, the same in numpy and in the kernel -- and none between the clipped kernel at clip 0, the search's candidate 0 and the plain
kernel: they are the same arithmetic in the same order.  The float64 sums are compared with the correctly rounded sum of the same
terms: `cols * 2^-52` relative (tests/quant_ref.py has the reasoning).  The searched index is compared with the reference's exactly: on
these inputs the reference's best two candidates differ by at least 4.9e-5 relative (printed and asserted below), the bound is at most
5.8e-11.
Shapes: row lengths 1, 9, 63, 64, 65, 1024 (a wave per row, 20 rows: two workgroups), 1025, 4099 and 262144 (a workgroup per row; 1025
rows start off the 16-byte grid, 4099 and 262144 on and off it), the rows of test_gpu_quant chosen to break things, 2, 4 and 8 bits."""
import numpy as np
import pytest
import torch

import qat_ref as qat
import quant_ref as qref
import test_gpu_quant as tq
import test_gpu_trainer as tt
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import ops
from wakeword_jupyterlab_amd.optim import FusedAdam

pytestmark = pytest.mark.gpu
DEV = tt.DEV
BITS = (2, 4, 8)
GAUSS_COLS = (1, 9, 63, 64, 65, 1024, 1025, 4099)
N_GAUSS = len(GAUSS_COLS) + 1
_np, _bits_equal = tq._np, tq._bits_equal


# ======================================================================================================================================
# inputs and references: computed once, shared, never modified
# ======================================================================================================================================
def _make_inputs():
    """[(numpy weight, per_channel)]: the seeded Gaussian rows (sigma 0.05, seed 1234) of every row length, then the special rows at a wave
    per row (9, 65) and a workgroup per row (1025), per channel and -- the first four of 4099 columns -- per tensor."""
    rng = np.random.default_rng(1234)
    items = [((rng.standard_normal((20 if c <= 1025 else 3, c)) * 0.05).astype(np.float32), True) for c in GAUSS_COLS]
    items.append(((rng.standard_normal(262144) * 0.05).astype(np.float32), False))
    items += [(tq._special_rows(c, rng), True) for c in (9, 65, 1025)]
    items += [(row.copy(), False) for row in tq._special_rows(4099, rng)[[0, 2, 4, 6]]]
    items.append((np.array([[0.0], [-0.375], [3e38], [np.nan]], np.float32), True))          # single-element rows
    return items


_CACHE = {}


def _inputs():
    if "items" not in _CACHE:
        _CACHE["items"] = _make_inputs()
        _CACHE["dev"] = [torch.from_numpy(w).to(DEV) for w, _ in _CACHE["items"]]
    return _CACHE["items"], _CACHE["dev"]


def _modes():
    return [pc for _, pc in _inputs()[0]]


def _rows2d(i):
    w, pc = _inputs()[0][i]
    return w.reshape(qref.groups(w.shape, pc))


def _random_clips(bits):
    key = ("clips", bits)
    if key not in _CACHE:
        rng = np.random.default_rng(100 + bits)
        host = [rng.integers(0, qat.CLIP_STEPS, _rows2d(i).shape[0]).astype(np.uint8) for i in range(len(_inputs()[0]))]
        _CACHE[key] = (host, [torch.from_numpy(c).to(DEV) for c in host])
    return _CACHE[key]


def _plain(bits):
    key = ("plain", bits)
    if key not in _CACHE:
        _CACHE[key] = ops.quantize_weights(_inputs()[1], bits=bits, per_channel=_modes())
        torch.cuda.synchronize()
    return _CACHE[key]


def _clipped(bits):
    """The clipped kernel under the seeded random indices, and its reference."""
    key = ("clipped", bits)
    if key not in _CACHE:
        host, dev = _random_clips(bits)
        ours = ops.quantize_weights_clip(_inputs()[1], dev, bits=bits, per_channel=_modes())
        torch.cuda.synchronize()
        _CACHE[key] = (ours, [qat.quantize_clip(w, c, bits, pc) for (w, pc), c in zip(_inputs()[0], host)])
    return _CACHE[key]


def _searched(bits):
    key = ("searched", bits)
    if key not in _CACHE:
        ours = ops.quant_clip_search(_inputs()[1], bits=bits, per_channel=_modes())
        torch.cuda.synchronize()
        _CACHE[key] = (ours, [qat.search(w, bits, pc) for w, pc in _inputs()[0]])
    return _CACHE[key]


def _name(i, bits):
    rows, cols = _rows2d(i).shape
    return f"tensor {i} ({rows} x {cols}, int{bits})"


# ======================================================================================================================================
# 1, 2: the clipped quantiser
# ======================================================================================================================================
@pytest.mark.parametrize("bits", BITS)
def test_clip_zero_is_the_plain_kernel_byte_for_byte(bits):
    _, dev = _inputs()
    zeros = [torch.zeros(_rows2d(i).shape[0], device=DEV, dtype=torch.uint8) for i in range(len(dev))]
    ours = ops.quantize_weights_clip(dev, zeros, bits=bits, per_channel=_modes())
    torch.cuda.synchronize()
    assert len(dev) > 16                                           # more than one launch
    for i, (got, want) in enumerate(zip(ours, _plain(bits))):
        for slot, what in enumerate(("q", "scale", "deq", "err", "bad")):
            assert _bits_equal(_np(got[slot]), _np(want[slot])), (_name(i, bits), what)
        assert not _np(got[5]).any(), (_name(i, bits), "sat")


@pytest.mark.parametrize("bits", BITS)
def test_clipped_kernel_equals_the_reference(bits):
    ours, refs = _clipped(bits)
    saturated = 0
    for i, ((q, scale, deq, err, bad, sat), want) in enumerate(zip(ours, refs)):
        name = _name(i, bits)
        for got, key in ((scale, "scale"), (q, "q"), (deq, "deq"), (sat, "sat"), (bad, "bad")):
            assert _bits_equal(_np(got), want[key]), (name, key)
        tq._check_err(name, _np(err), want["err"], _rows2d(i).shape[1])
        assert int(np.abs(_np(q).astype(int)).max()) <= qref.qmax_of(bits), name
        saturated += int(_np(sat).sum())
    assert saturated > 0


def test_a_clip_index_past_the_last_candidate_counts_as_the_last():
    _, dev = _inputs()
    pick = [2, 6, 7]                                               # 20 x 63, 20 x 1025, 3 x 4099
    rows = [_rows2d(i).shape[0] for i in pick]
    outs = [ops.quantize_weights_clip([dev[i] for i in pick], [torch.full((r,), v, device=DEV, dtype=torch.uint8) for r in rows], bits=4,
                                      per_channel=True) for v in (47, 48, 255)]
    torch.cuda.synchronize()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert all(_bits_equal(_np(x), _np(y)) for x, y in zip(a, b))
    assert _bits_equal(_np(outs[0][0][1]), qat.scales(_rows2d(2), np.full(20, 47), 4))


def test_clipped_outputs_stay_inside_their_ranges_at_any_alignment_and_may_be_null():
    """Guarded buffers at every phase of the 16-byte grid: the bytes of the aligned call, nothing written outside; with every optional
    output NULL the scale alone is written, the same."""
    items, dev = _inputs()
    pick = [1, 4, 5, 6, 7, 8, 11, 12]                              # 9, 65, 1024, 1025, 4099 and 262144 columns, special rows at 1025 and 4099
    host, clips = _random_clips(4)
    weights, outs, guards = [], [[] for _ in range(7)], []
    for j, i in enumerate(pick):
        w, pc = items[i]
        rows = _rows2d(i).shape[0]
        wv, wi = tq._guarded(w.size, torch.float32, 1 + j % 4)
        wv.copy_(dev[i].reshape(-1))
        weights.append(wv.view(w.shape))
        guards.append(wi)
        for slot, (numel, dtype, lead) in enumerate(((rows, torch.float32, 1 + j % 3), (w.size, torch.int8, 1 + j % 5), (w.size, torch.float32, 2 + j % 4),
                                                     (3 * rows, torch.float64, 1 + j % 2), (rows, torch.int32, 3 + j % 3), (rows, torch.int32, 1 + j % 4))):
            v, ok = tq._guarded(numel, dtype, lead)
            outs[slot].append(v.view(w.shape) if slot in (1, 2) else v)
            guards.append(ok)
        cv = torch.full((rows + 5,), 7, device=DEV, dtype=torch.uint8)
        cv[1 + j % 3:1 + j % 3 + rows] = clips[i]
        outs[6].append(cv[1 + j % 3:1 + j % 3 + rows])
    modes = [items[i][1] for i in pick]
    tab = ops.quant_clip_table(weights, outs[0], outs[6], outs[1], outs[2], outs[3], outs[4], outs[5], per_channel=modes)
    ops.quantize_weights_clip_launch(tab, DEV, 4)
    torch.cuda.synchronize()
    assert all(g() for g in guards)
    shared = _clipped(4)[0]
    for j, i in enumerate(pick):
        for slot, ref_slot in enumerate((1, 0, 2, 3, 4, 5)):       # (scale, q, deq, err, bad, sat) <- (q, scale, deq, err, bad, sat)
            assert _bits_equal(_np(outs[slot][j]).reshape(-1), _np(shared[i][ref_slot]).reshape(-1)), (i, slot)
    scales = [torch.zeros_like(s) for s in outs[0]]
    ops.quantize_weights_clip_launch(ops.quant_clip_table(weights, scales, outs[6], per_channel=modes), DEV, 4)
    torch.cuda.synchronize()
    assert all(g() for g in guards) and all(_bits_equal(_np(a), _np(b)) for a, b in zip(scales, outs[0]))


# ======================================================================================================================================
# 3: the search
# ======================================================================================================================================
@pytest.mark.parametrize("bits", BITS)
def test_search_equals_the_reference(bits):
    ours, refs = _searched(bits)
    for i, ((clip, scale, cand), want) in enumerate(zip(ours, refs)):
        name, (rows, cols) = _name(i, bits), _rows2d(i).shape
        clip, scale, cand = _np(clip), _np(scale), _np(cand)
        assert cand.shape == (rows, qat.CLIP_STEPS) and np.isfinite(cand).all(), name
        assert _bits_equal(cand[:, 0], _np(_plain(bits)[i][3])[:, 1]), f"{name}: candidate 0 is the plain kernel's error sum"
        bound = cols * 2.0 ** -52
        rel = np.abs(cand - want["cand_err"]) / np.where(want["cand_err"] == 0.0, 1.0, want["cand_err"])
        print(f"{name}: worst relative difference of a candidate's error {rel.max():.3e} (bound {bound:.3e}), smallest gap {want['gap'].min():.3e}")
        assert np.all(rel <= bound) and np.all(cand[want["cand_err"] == 0.0] == 0.0), f"{name}: {rel.max():.3e} > {bound:.3e}"
        assert clip.dtype == np.uint8 and np.array_equal(clip, cand.argmin(axis=1)), f"{name}: the first argmin of the written errors"
        assert _bits_equal(scale, qat.scales(_rows2d(i), clip, bits)), name
        if i < N_GAUSS:                                            # the seeded Gaussian rows: the reference's argmin, no row excused
            assert want["gap"].min() >= 1e3 * bound, f"{name}: the reference's best two candidates are too close to tell apart"
            assert np.array_equal(clip, want["clip"]) and _bits_equal(scale, want["scale"]), name
    if bits <= 4:
        assert max(int(_np(c).max()) for c, _, _ in ours[:N_GAUSS]) > 0


def test_search_edge_rows_and_null_cand_err():
    items, dev = _inputs()
    ours, _ = _searched(4)
    specials = N_GAUSS + 1                                         # the special rows at 65 columns
    clip = _np(ours[specials][0])
    assert clip[0] == 0 and clip[7] == 0 and clip[8] == 0          # the zero row, all NaN, all Inf: every candidate's error is 0
    assert not _np(ours[-1][0]).any()                              # single-element rows: zero, one value, 3e38, NaN
    assert not _np(ours[0][0]).any()                               # ... and the Gaussian ones
    pick = [0, 3, 6, 7, 8, N_GAUSS + 2]
    lean = ops.quant_clip_search([dev[i] for i in pick], bits=4, per_channel=[items[i][1] for i in pick], cand_err=False)
    torch.cuda.synchronize()
    for i, (c, s, e) in zip(pick, lean):
        assert e is None and _bits_equal(_np(c), _np(ours[i][0])) and _bits_equal(_np(s), _np(ours[i][1])), i
    again = ops.quant_clip_search(dev, bits=4, per_channel=_modes())
    torch.cuda.synchronize()
    assert all(_bits_equal(_np(x), _np(y)) for a, b in zip(again, ours) for x, y in zip(a, b))       # the same call, the same bytes


# ======================================================================================================================================
# 4: the straight-through estimator
# ======================================================================================================================================
@pytest.mark.parametrize("bits", BITS)
def test_ste_equals_the_numpy_mask(bits):
    items, dev = _inputs()
    ours, refs = _clipped(bits)
    rng = np.random.default_rng(7 + bits)
    grads_host, grads = [], []
    for i, (w, _) in enumerate(items):
        g = rng.standard_normal(w.shape).astype(np.float32)
        flat, moved = g.reshape(-1), qat.ste(w, refs[i]["scale"], np.ones(w.shape, np.float32), bits, items[i][1]).reshape(-1) == 0.0
        flat[::7] = np.nan                                         # NaN gradients everywhere, saturated elements among them
        flat[3::11] = -0.0
        if moved.any():
            flat[np.flatnonzero(moved)[0]] = np.nan
        grads_host.append(g)
        grads.append(torch.from_numpy(g.copy()).to(DEV))
    scales = [o[1] for o in ours]
    first = [g.clone() for g in grads]
    ops.quant_ste_(dev, scales, first, bits=bits, per_channel=_modes())
    ops.quant_ste_(dev, scales, grads, bits=bits, per_channel=_modes())
    torch.cuda.synchronize()
    cut = cut_nan = kept_nonfinite = 0
    for i, (w, pc) in enumerate(items):
        want = qat.ste(w, refs[i]["scale"], grads_host[i], bits, pc)
        assert _bits_equal(_np(grads[i]), want) and _bits_equal(_np(first[i]), want), _name(i, bits)
        changed = want.view(np.int32) != grads_host[i].view(np.int32)
        cut += int(changed.sum())
        cut_nan += int(np.isnan(grads_host[i][changed]).sum())
        kept_nonfinite += int((~np.isfinite(w)).sum())
        assert not changed[~np.isfinite(w)].any()                  # a non-finite w: g untouched
        assert not np.signbit(want[changed]).any() and not want[changed].any()                      # +0.0
    assert kept_nonfinite > 0
    if bits <= 4:
        assert sum(int(_np(o[5]).sum()) for o in ours) > 0 and cut > 0 and cut_nan > 0               # not vacuous


def test_ste_stays_inside_its_range_off_the_grid():
    items, dev = _inputs()
    ours, refs = _clipped(4)
    for i in (6, 7, 8):                                            # 1025, 4099, 262144 columns
        w, pc = items[i]
        for lead in (1, 2, 3, 4):
            wv, w_ok = tq._guarded(w.size, torch.float32, lead)
            gv, g_ok = tq._guarded(w.size, torch.float32, 5 - lead)
            wv.copy_(dev[i].reshape(-1))
            gv.fill_(1.5)
            ops.quant_ste_([wv.view(w.shape)], [ours[i][1]], [gv.view(w.shape)], bits=4, per_channel=pc)
            torch.cuda.synchronize()
            assert w_ok() and g_ok() and _bits_equal(_np(gv).reshape(w.shape), qat.ste(w, refs[i]["scale"], np.full(w.shape, 1.5, np.float32), 4, pc))


# ======================================================================================================================================
# WeightQuant(clip="mse")
# ======================================================================================================================================
def _golden_master(arch):
    """The synthetic seed-1234 weights (Gaussian rows: a clipped scale saturates some of them) in a train-mode model."""
    model, sd = tq._golden_model(arch)
    return model.train(), sd


def test_weight_quant_mse_calibrates_updates_reports_and_round_trips(tmp_path):
    model, sd = _golden_master("simple")
    wq = pkg.WeightQuant(model, bits=4, clip="mse")
    assert wq.clip_mode == "mse" and wq.n_calibrations == 1 and wq.n_updates == 1 and list(wq.clip) == wq.quantized
    clips = {k: _np(v) for k, v in wq.clip.items()}
    for k in wq.quantized:
        if sd[k].shape[0] <= 64:                                   # the convolutions and fc: the reference's search is a Python loop
            want = qat.search(sd[k], 4, True)
            assert want["gap"].min() >= 1e-9 and np.array_equal(clips[k], want["clip"]), k      # 1e-9: far above the summation bound
        ref = qat.quantize_clip(sd[k], clips[k], 4, True)
        assert _bits_equal(_np(wq.q[k]), ref["q"]) and _bits_equal(_np(wq.scale[k]), ref["scale"]), k
        assert _bits_equal(_np(dict(wq.model.named_parameters())[k]), ref["deq"]), k
    assert max(int(c.max()) for c in clips.values()) > 0
    # the report: one copy, the new columns behind the same buffer
    rep, plain = wq.report(), pkg.WeightQuant(model, bits=4).report()
    assert rep.clip == "mse" and rep.totals["saturated"] > 0 and 17 / 64 <= rep.totals["clip_min"] < 1.0 and rep.totals["clip_mean"] < 1.0
    assert rep.totals["sqnr_db"] > plain.totals["sqnr_db"] and "saturated" in str(rep) and "saturated" not in str(plain)
    for t in rep.tensors:
        ref = qat.quantize_clip(sd[t["name"]], clips[t["name"]], 4, True)
        assert t["saturated"] == int(ref["sat"].sum()) and t["clip_min"] == float(qat.fractions(clips[t["name"]]).min())
    # update(): the stored indices, no search; the fast form leaves the kept biases alone
    with torch.no_grad():
        model.conv2.weight.mul_(1.25)
        model.fc.bias.add_(0.5)
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        wq.update(weights_only=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == allocated and wq.n_calibrations == 1 and wq.n_updates == 2
    ref = qat.quantize_clip(_np(model.conv2.weight), clips["conv2.weight"], 4, True)
    assert _bits_equal(_np(wq.model.conv2.weight), ref["deq"]) and _bits_equal(_np(wq.clip["conv2.weight"]), clips["conv2.weight"])
    assert not torch.equal(wq.model.fc.bias, model.fc.bias)
    wq.update()
    assert torch.equal(wq.model.fc.bias, model.fc.bias)
    wq.calibrate()
    assert wq.n_calibrations == 2 and wq.n_updates == 4
    # state and package: `clip` travels, the loader rebuilds from q * scale alone
    state = wq.state_dict()
    assert sorted(state) == sorted(["bits", "per_channel", "quantize_bias", "q", "scale", "float", "clip"])
    path = str(tmp_path / "mse.pth")
    pkg.save_quantized_package(wq, path)
    fresh = pkg.SimpleWakewordModel().to(DEV)
    st = pkg.load_quantized_package(path, fresh)["quantized"]
    assert list(st["clip"]) == wq.quantized and all(v.dtype == torch.uint8 for v in st["clip"].values())
    assert all(_bits_equal(_np(a), _np(b)) for a, b in zip(fresh.parameters(), wq.model.parameters()))
    twin = pkg.WeightQuant(tt._model("simple", seed=3), bits=8)
    twin.load_state_dict(state)
    assert twin.clip_mode == "mse" and twin.bits == 4 and all(_bits_equal(_np(a), _np(b)) for a, b in zip(twin.model.parameters(), wq.model.parameters()))
    assert all(_bits_equal(_np(twin.clip[k]), _np(wq.clip[k])) for k in wq.quantized)


# ======================================================================================================================================
# 5, 6, 7: the trainer
# ======================================================================================================================================
B = 8
NAMES = tq.NAMES + ("quantize_weights_clip_launch", "quant_clip_search_launch", "quant_ste_launch", "distill_loss_into")


@pytest.mark.parametrize("arch, T, clip, teacher", [("simple", 32, "max", False), ("simple", 32, "mse", False), ("full", 32, "mse", False),
                                                     ("full", 32, "max", False), ("simple", 8, "mse", False), ("simple", 32, "mse", True)])
def test_qat_step_equals_its_parts(arch, T, clip, teacher):
    lr, wd = pkg.TrainingConfig.LEARNING_RATE, 1e-5
    model, sd = _golden_master(arch)
    wq = pkg.WeightQuant(model, bits=4, clip=clip)
    big = tt._model("full", seed=5).eval() if teacher else None
    trainer = pkg.WakewordTrainer(model, DEV, quant=wq, qat=True, teacher=big)
    x, y = tt._batch(B, T, seed=3)
    master = {k: p.detach().clone() for k, p in model.named_parameters()}
    torch.manual_seed(77)
    trainer.step(x, y)
    torch.cuda.synchronize()
    # ---- a train-mode copy of quant.model carrying the master's biases, through the module's autograd path, same seed ----
    twin = tt.MODELS[arch]().to(DEV).train()
    own = dict(wq.model.named_parameters())
    with torch.no_grad():
        for k, p in twin.named_parameters():
            p.copy_(own[k] if k in wq.q else master[k])
            if k in wq.q:                                          # the step quantised the weights it was given
                ref = qref.quantize(_np(master[k]), 4, True) if clip == "max" else qat.quantize_clip(_np(master[k]), _np(wq.clip[k]), 4, True)
                assert _bits_equal(_np(p), ref["deq"]), k
    torch.manual_seed(77)
    out = twin(x)
    assert torch.equal(trainer.last_logits[:B], out.detach())
    dlogits = trainer._dlogits[:B].clone() if teacher else ops.ce_loss(out.detach(), y)[1]
    out.backward(gradient=dlogits)
    # ---- the mask, in numpy; FusedAdam on a clone of the master ----
    clone = tt.MODELS[arch]().to(DEV)
    cut = 0
    with torch.no_grad():
        for k, p in clone.named_parameters():
            p.copy_(master[k])
    for (k, p), tp in zip(clone.named_parameters(), twin.parameters()):
        g = _np(tp.grad)
        if clip == "mse" and k in wq.q:
            masked = qat.ste(_np(master[k]), _np(wq.scale[k]), g, 4, True)
            cut += int((masked.view(np.int32) != g.view(np.int32)).sum())
            g = masked
        p.grad = torch.from_numpy(g).to(DEV)
    named = dict(model.named_parameters())
    for k, p in clone.named_parameters():
        assert _bits_equal(_np(named[k].grad), _np(p.grad)), k
    if clip == "mse":
        assert wq.report().totals["saturated"] > 0 and cut > 0      # the mask did something
    opt = FusedAdam(clone.parameters(), lr=lr, weight_decay=wd)
    opt.step()
    torch.cuda.synchronize()
    for k, p in clone.named_parameters():
        assert _bits_equal(_np(named[k]), _np(p)), k
        assert not _bits_equal(_np(named[k]), _np(master[k])), k


def test_a_quantiser_without_qat_leaves_training_as_it_was():
    x, y = tt._batch(B, 32, seed=6)
    runs = []
    for with_quant in (False, True):
        model, _ = _golden_master("simple")
        trainer = pkg.WakewordTrainer(model, DEV, quant=pkg.WeightQuant(model) if with_quant else None)
        assert trainer.qat is False
        torch.manual_seed(11)
        for _ in range(3):
            trainer.step(x, y)
        torch.cuda.synchronize()
        runs.append(tt._state_of(model, trainer.optimizer))
    for role in "pmv":
        for k in runs[0][role]:
            assert _bits_equal(runs[0][role][k], runs[1][role][k]), (role, k)


@pytest.mark.parametrize("clip", ["max", "mse"])
def test_qat_step_launches_waits_and_allocations(monkeypatch, clip):
    """One more launch than a plain step under "max", two more under "mse"; no wait; no allocation after the first step."""
    x, y = tt._batch(B, 8, seed=6)
    model, _ = _golden_master("full")
    wq = pkg.WeightQuant(model, bits=4, clip=clip)
    trainer = pkg.WakewordTrainer(model, DEV, quant=wq, qat=True, qat_calibrate=None)
    for _ in range(2):
        trainer.step(x, y)
    torch.cuda.synchronize()
    calls = tq._record(monkeypatch, NAMES)
    torch.cuda.set_sync_debug_mode("error")
    try:
        trainer.step(x, y)
        before = torch.cuda.memory_allocated()
        trainer.step(x, y)
        after = torch.cuda.memory_allocated()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        monkeypatch.undo()
    assert before == after
    plain = ["train_forward_into", "ce_loss_into", "train_backward_into", "adam_launch"]
    want = (["quantize_weights_launch"] + plain if clip == "max" else
            ["quantize_weights_clip_launch"] + plain[:3] + ["quant_ste_launch", "adam_launch"])
    assert calls == want * 2 and wq.n_calibrations == (1 if clip == "mse" else 0)
    torch.cuda.synchronize()
    assert ops.read_loss_stats(trainer.train_stats)["batches"] == 4


def test_qat_calibrate_schedules_and_composition(tmp_path):
    x, y = tt._batch(B, 8, seed=9)
    loader = [(x, y)] * 3
    for schedule, want in (("epoch", 3), (2, 3), (None, 1)):        # construction, then: two epochs; before steps 2 and 4 (from 0); never
        model, _ = _golden_master("simple")
        wq = pkg.WeightQuant(model, bits=4, clip="mse")
        trainer = pkg.WakewordTrainer(model, DEV, quant=wq, qat=True, qat_calibrate=schedule, evaluate="quant", max_grad_norm=1.0,
                                      average=pkg.WeightAverage(model, decay=0.9), checkpoint_path=str(tmp_path / "best.pth"))
        torch.manual_seed(1)
        for _ in range(2):
            loss, acc = trainer.train_epoch(loader[:2] if schedule == 2 else loader)
            assert np.isfinite(loss)
        if schedule == 2:
            trainer.step(x, y)
        assert wq.n_calibrations == want, schedule
        got = trainer.validate([(x, y)])                           # the full update: quant.model carries the master's biases again
        assert all(torch.equal(dict(wq.model.named_parameters())[k], dict(model.named_parameters())[k]) for k in wq.kept) and np.isfinite(got[0])
    with pytest.raises(NotImplementedError, match="select"):
        trainer.select = pkg.HardSelect(4)
    state = wq.state_dict()                                         # a state without `clip`: the quantiser turns "max", with new buffers
    del state["clip"]
    wq.load_state_dict(state)
    model.train()
    trainer.step(x, y)
    assert wq.clip_mode == "max" and trainer._ste_tables == [] and bool(torch.isfinite(trainer.last_loss))
    max_q = pkg.WeightQuant(model, bits=4)                          # "max": the schedule is ignored
    t2 = pkg.WakewordTrainer(model, DEV, quant=max_q, qat=True, qat_calibrate=1)
    model.train()
    for _ in range(3):
        t2.step(x, y)
    assert max_q.n_calibrations == 0 and max_q.n_updates == 4
