"""Weight quantisation on the GPU (quant_kernel in csrc/ww_quant.hip): the kernel against the numpy restatement
of its rule (tests/quant_ref.py) bit for bit, WeightQuant's fake-quant model against the same class loaded with the reference's weights,
the package round trip, and WakewordTrainer(quant=, evaluate="quant").

Tolerances: none on q, scale, deq and bad, and none on the largest error -- every step of the rule is one correctly rounded float32
operation, the same in numpy and in the kernel.  The two float64 sums are compared with the correctly rounded sum of the same terms:
`cols * 2^-52` relative, the bound of adding `cols` non-negative float64 terms in any order (quant_ref.py has the reasoning).
Shapes: every row length at which the mapping changes (one lane, under / at / over a wave, several elements per lane, the wave path's last
length 1024 is covered by 576 and 1025 around the switch to a workgroup per row), rows 1 .. 64 (more than one workgroup: 16 rows each)."""
import numpy as np
import pytest
import torch

import quant_ref as qref
import test_gpu_trainer as tt
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import ops, quant

pytestmark = pytest.mark.gpu
DEV = tt.DEV
BITS = (2, 4, 8)
PC_COLS, PC_ROWS = (1, 9, 63, 64, 65, 288, 576, 1025), (1, 2, 5, 64)
PT_COLS = (1, 63, 65, 4097, 262144)


def _np(t):
    return t.detach().cpu().numpy()


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ======================================================================================================================================
# inputs: the shape grid with rows of very different magnitude, and rows chosen to break things
# ======================================================================================================================================
def _special_rows(cols, rng):
    """[10, cols]: an all-zero row; one non-zero; exact ties under a scale of 1; a denormal amax; amax near 3e38; -0.0 among ordinary
    values; NaN and +-Inf mixed into a finite row; all NaN; all +Inf; a row of equal values."""
    base = rng.standard_normal((10, cols)).astype(np.float32)
    base[0] = 0.0
    base[1] = 0.0
    base[1, cols // 2] = -0.375
    base[2] = 0.0
    ties = [127.0, 0.5, 1.5, 2.5, -0.5, -1.5]
    base[2, :min(cols, 6)] = ties[:min(cols, 6)]
    base[3] = (base[3] * np.float32(2.0 ** -130)).astype(np.float32)
    base[3, 0] = np.float32(2.0 ** -127)
    base[4] = (base[4] / np.abs(base[4]).max() * np.float32(3e38)).astype(np.float32)
    base[5, ::3] = -0.0
    base[6, 0::5] = np.nan
    if cols > 1:
        base[6, 1::7] = np.inf
    if cols > 2:
        base[6, 2::11] = -np.inf
    base[7] = np.nan
    base[8] = np.inf
    base[9] = -1.25
    return base


def _grid_tensor(rows, cols, rng):
    w = (rng.standard_normal((rows, cols)) * 10.0 ** rng.uniform(-6, 3, (rows, 1))).astype(np.float32)
    if rows * cols >= 9:
        flat = w.reshape(-1)
        flat[rng.integers(0, flat.size)] = -0.0
        flat[rng.integers(0, flat.size)] = np.nan
    return w


def _make_inputs():
    """[(numpy weight, per_channel)]: 32 grid tensors and 4 tensors of special rows per channel; 5 grid tensors and 20 special rows per tensor."""
    rng = np.random.default_rng(20240)
    items = [(_grid_tensor(r, c, rng), True) for c in PC_COLS for r in PC_ROWS]
    items += [(_special_rows(c, rng), True) for c in (9, 65, 576, 1025)]
    items += [(_grid_tensor(1, c, rng).reshape(-1), False) for c in PT_COLS]
    for c in (65, 4097):
        items += [(row.copy(), False) for row in _special_rows(c, rng)]
    return items


_CACHE = {}


def _inputs():
    if "items" not in _CACHE:
        _CACHE["items"] = _make_inputs()
        _CACHE["dev"] = [torch.from_numpy(w).to(DEV) for w, _ in _CACHE["items"]]
    return _CACHE["items"], _CACHE["dev"]


def _reference(bits):
    """The reference of every input at `bits`: computed once, shared, never modified."""
    key = ("ref", bits)
    if key not in _CACHE:
        _CACHE[key] = [qref.quantize(w, bits, pc) for w, pc in _inputs()[0]]
    return _CACHE[key]


def _ours(bits):
    key = ("ours", bits)
    if key not in _CACHE:
        items, dev = _inputs()
        _CACHE[key] = ops.quantize_weights(dev, bits=bits, per_channel=[pc for _, pc in items])
        torch.cuda.synchronize()
    return _CACHE[key]


def _check_err(name, got, want, cols):
    got, want = np.asarray(got, np.float64).reshape(-1, 3), np.asarray(want, np.float64).reshape(-1, 3)
    assert np.isfinite(got).all(), name
    assert np.array_equal(got[:, 2], want[:, 2]), f"{name}: the largest error is exact"
    bound = cols * 2.0 ** -52
    for j, what in ((0, "sum w^2"), (1, "sum err^2")):
        rel = np.abs(got[:, j] - want[:, j]) / np.where(want[:, j] == 0.0, 1.0, want[:, j])
        print(f"{name} {what}: worst relative difference {rel.max():.3e} (bound {bound:.3e})")
        assert np.all(rel <= bound), f"{name} {what}: {rel.max():.3e} > {bound:.3e}"
        assert np.all(got[want[:, j] == 0.0, j] == 0.0), f"{name} {what}: a zero sum is exactly zero"


@pytest.mark.parametrize("bits", BITS)
def test_kernel_equals_the_reference_bit_for_bit(bits):
    items, _ = _inputs()
    assert len(items) == 32 + 4 + 5 + 20                           # 61 tensors: launches of 16, 16, 16 and 13
    for i, ((w, pc), (q, scale, deq, err, bad), want) in enumerate(zip(items, _ours(bits), _reference(bits))):
        rows, cols = qref.groups(w.shape, pc)
        name = f"tensor {i} ({rows} x {cols}, {'rows' if pc else 'tensor'}, int{bits})"
        assert q.dtype == torch.int8 and q.shape == w.shape and deq.shape == w.shape and tuple(err.shape) == (rows, 3), name
        assert _bits_equal(_np(scale), want["scale"]), name
        assert _bits_equal(_np(q), want["q"]), name
        assert _bits_equal(_np(deq), want["deq"]), name
        assert _bits_equal(_np(bad), want["bad"]), name
        assert int(np.abs(_np(q).astype(int)).max()) <= qref.qmax_of(bits), name
        _check_err(name, _np(err), want["err"], cols)


def test_the_rows_chosen_to_break_things_did_what_they_were_chosen_for():
    """The special rows through the kernel's own output: so that the bit-equality above is known to have covered them."""
    items, _ = _inputs()
    i = 32 + 1                                                      # the special rows at 65 columns, one scale per row
    q, scale, deq, err, bad = (_np(t) for t in _ours(8)[i])
    tiny = np.float32(2.0 ** -126)
    assert scale[0] == tiny and not q[0].any() and not deq[0].any() and not err[0].any()
    assert np.count_nonzero(q[1]) == 1 and q[1, 32] == -127 and abs(float(deq[1, 32]) + 0.375) <= 0.375 * 2.0 ** -22
    assert scale[2] == 1.0 and q[2, :6].tolist() == [127, 0, 2, 2, 0, -2]                            # ties to even
    assert scale[3] == tiny and np.abs(q[3].astype(int)).max() <= 1 and err[3, 0] > 0.0              # a denormal amax: floored, not flushed
    assert np.isfinite(deq[4]).all() and np.abs(q[4].astype(int)).max() == 127 and np.isfinite(err[4]).all()
    assert not np.signbit(deq[5, ::3]).any() and not q[5, ::3].any()                                 # -0.0 -> q 0 -> +0.0
    w6 = items[i][0][6]
    assert bad[6] == int((~np.isfinite(w6)).sum()) > 0 and not q[6][~np.isfinite(w6)].any() and np.isfinite(deq[6]).all()
    assert np.abs(q[6].astype(int)).max() == 127                                                     # amax over the finite elements alone
    for r in (7, 8):
        assert bad[r] == 65 and scale[r] == tiny and not q[r].any() and not deq[r].any() and not err[r].any()
    assert np.all(q[9] == -127) and bad[9] == 0
    assert bad[:6].tolist() == [0] * 6


@pytest.mark.parametrize("n, launches", [(1, 1), (16, 1), (17, 2)])
def test_call_sizes(monkeypatch, n, launches):
    items, dev = _inputs()
    pick = [(5 * k + 3) % 32 for k in range(n)]                     # a mix of row lengths in one table
    pick[-1] = 32 + 4 + 4                                           # ... and the 262144-element tensor among them
    calls = []
    real = ops.quantize_weights_launch
    monkeypatch.setattr(ops, "quantize_weights_launch", lambda table, *a, **k: (calls.append(len(table)), real(table, *a, **k))[1])
    got = ops.quantize_weights([dev[i] for i in pick], bits=8, per_channel=[items[i][1] for i in pick])
    torch.cuda.synchronize()
    assert len(calls) == launches and sum(calls) == n and max(calls) <= 16
    for i, out in zip(pick, got):
        for ours, shared in zip(out, _ours(8)[i]):
            assert _bits_equal(_np(ours), _np(shared)), i           # the bytes do not depend on what else is in the table


def _guarded(numel, dtype, lead):
    """A view of `numel` elements starting `lead` elements into a buffer filled with a sentinel, and the check that only the view changed."""
    sentinel = {torch.float32: 7.5, torch.float64: 7.5, torch.int8: 77, torch.int32: 7777777}[dtype]
    buf = torch.full((lead + numel + 67,), sentinel, device=DEV, dtype=dtype)
    view = buf[lead:lead + numel]

    def intact():
        return bool(torch.all(buf[:lead] == sentinel)) and bool(torch.all(buf[lead + numel:] == sentinel))
    return view, intact


def test_outputs_stay_inside_their_ranges_at_any_alignment_and_repeat():
    """Outputs cut from guarded buffers at every phase of the 16-byte grid, inputs too: the bytes are those of the aligned call, nothing
    outside a range is written, and a second call writes the same bytes."""
    items, _ = _inputs()
    pick = [3, 14, 27, 31, 32 + 3, 32 + 4 + 3, 32 + 4 + 4, 32 + 4 + 5 + 10 + 6]   # 64 x 1, 5 x 64, 64 x 576, 64 x 1025, specials 10 x 1025, 4097, 262144, a special 4097
    weights, outs, guards, modes = [], [[] for _ in range(5)], [], []
    for j, i in enumerate(pick):
        w, pc = items[i]
        rows, _ = qref.groups(w.shape, pc)
        wv, wi = _guarded(w.size, torch.float32, 1 + j % 4)
        wv.copy_(torch.from_numpy(w.reshape(-1)))
        weights.append(wv.view(w.shape))
        modes.append(pc)
        guards.append(wi)
        for slot, (numel, dtype, lead) in enumerate(((rows, torch.float32, 1 + j % 3), (w.size, torch.int8, 1 + j % 5), (w.size, torch.float32, 2 + j % 4),
                                                     (3 * rows, torch.float64, 1 + j % 2), (rows, torch.int32, 3 + j % 3))):
            v, ok = _guarded(numel, dtype, lead)
            outs[slot].append(v.view(w.shape) if slot in (1, 2) else v)
            guards.append(ok)
    ops.quantize_weights_into(weights, *outs, bits=4, per_channel=modes)
    torch.cuda.synchronize()
    first = [[_np(t).copy() for t in col] for col in outs]
    assert all(g() for g in guards)
    for j, i in enumerate(pick):
        for slot in range(5):
            shared = _ours(4)[i][(1, 0, 2, 3, 4)[slot]]            # (q, scale, deq, err, bad) -> (scale, q, deq, err, bad)
            assert _bits_equal(first[slot][j].reshape(-1), _np(shared).reshape(-1)), (i, slot)
    for col in outs[1:]:
        for t in col:
            t.fill_(1)                                             # whatever the outputs held is overwritten
    ops.quantize_weights_into(weights, *outs, bits=4, per_channel=modes)
    torch.cuda.synchronize()
    assert all(g() for g in guards)
    for slot in range(5):
        for j in range(len(pick)):
            assert _bits_equal(_np(outs[slot][j]), first[slot][j]), (slot, j)


@pytest.mark.parametrize("missing", ["q", "deq", "err", "bad", "all"])
def test_null_outputs_leave_the_others_unchanged(missing):
    items, dev = _inputs()
    pick = [9, 30, 31, 32 + 2, 32 + 4 + 3]                          # 2 x 63, 5 x 1025, 64 x 1025, specials 10 x 576, 4097 per tensor
    ws, modes = [dev[i] for i in pick], [items[i][1] for i in pick]
    names = ("scale", "q", "deq", "err", "bad")
    cols = {}
    for name, dtype in zip(names, (torch.float32, torch.int8, torch.float32, torch.float64, torch.int32)):
        if name == missing or (missing == "all" and name != "scale"):
            cols[name] = None
            continue
        cols[name] = []
        for w, pc in zip(ws, modes):
            rows, _ = ops.quant_groups(w, pc)
            shape = {"scale": (rows,), "q": w.shape, "deq": w.shape, "err": (rows, 3), "bad": (rows,)}[name]
            cols[name].append(torch.zeros(shape, device=DEV, dtype=dtype))
    ops.quantize_weights_into(ws, cols["scale"], cols["q"], cols["deq"], cols["err"], cols["bad"], bits=8, per_channel=modes)
    torch.cuda.synchronize()
    for name, slot in zip(names, (1, 0, 2, 3, 4)):
        if cols[name] is None:
            continue
        for i, t in zip(pick, cols[name]):
            assert _bits_equal(_np(t), _np(_ours(8)[i][slot])), (name, i)


def test_wrappers_refuse_before_any_launch(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "quantize_weights_launch", lambda *a, **k: calls.append(a))
    w = torch.zeros(4, 9, device=DEV)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.quantize_weights([w, w.t()])
    with pytest.raises(ValueError):
        ops.quantize_weights_into([w], [torch.zeros(3, device=DEV)])                      # 4 rows, 3 scales
    with pytest.raises(TypeError):
        ops.quantize_weights_into([w], [torch.zeros(4, device=DEV)], qs=[torch.zeros(4, 9, device=DEV)])   # q must be int8
    with pytest.raises(RuntimeError):
        ops.quantize_weights_into([w], [torch.zeros(4)])                                  # a scale on the CPU
    with pytest.raises(ValueError, match="empty"):
        ops.quantize_weights([torch.zeros(0, 9, device=DEV)])
    with pytest.raises(ValueError):
        ops.quantize_weights_into([w] * 17, [torch.zeros(4, device=DEV)] * 16)
    assert calls == []


# ======================================================================================================================================
# WeightQuant
# ======================================================================================================================================
def _golden_model(arch):
    sd = pkg.synth.make_state_dict(arch, seed=1234)                # the weights behind tests/golden/model_*_seed1234.npz
    model = tt.MODELS[arch]()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.to(DEV), sd


def _reference_model(arch, sd, **options):
    """The same class loaded with the reference-dequantised weights."""
    model = tt.MODELS[arch]()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in qref.fake_quant_state_dict(sd, **options).items()})
    return model.to(DEV).eval()


def _x(T, seed=5):
    return tt._batch(3, T, seed)[0]


def _host_sd(model):
    return {k: _np(v) for k, v in model.state_dict().items()}


@pytest.mark.parametrize("arch, options", [("simple", dict(bits=8, per_channel=True, quantize_bias=False)),
                                           ("full", dict(bits=8, per_channel=True, quantize_bias=False)),
                                           ("simple", dict(bits=4, per_channel=False, quantize_bias=True)),
                                           ("full", dict(bits=6, per_channel=True, quantize_bias=True))])
def test_fake_quant_model_equals_the_reference_weights_bit_for_bit(arch, options):
    model, sd = _golden_model(arch)
    wq = pkg.WeightQuant(model, **options)
    assert wq.n_updates == 1 and type(wq.model) is type(model) and not wq.model.training and model.training
    assert all(not p.requires_grad and p.grad is None for p in wq.model.parameters())
    want = qref.fake_quant_state_dict(sd, **options)
    for k, p in wq.model.named_parameters():
        assert _bits_equal(_np(p), want[k]), k
        if k in wq.q:
            ref = qref.quantize(sd[k], options["bits"], options["per_channel"] and sd[k].ndim >= 2)
            assert _bits_equal(_np(wq.q[k]), ref["q"]) and _bits_equal(_np(wq.scale[k]), ref["scale"]), k
    assert all(_bits_equal(_np(p), sd[k]) for k, p in model.named_parameters())           # the source is only read
    judge = _reference_model(arch, sd, **options)
    with torch.no_grad():
        for T in (8, 32):
            x = _x(T)
            assert _bits_equal(_np(wq.model(x)), _np(judge(x))), T
        raw = model.eval()(x)
    assert not torch.equal(raw, wq.model(x))                       # ... and they are not the float32 model's logits
    # the report, against the reference's float64 sums
    rep = wq.report()
    assert [t["name"] for t in rep.tensors] == wq.quantized and rep.totals["nonfinite"] == 0
    assert rep.totals["float_bytes"] == sum(4 * sd[k].size for k in wq.kept)
    for t in rep.tensors:
        ref = qref.quantize(sd[t["name"]], options["bits"], options["per_channel"] and sd[t["name"]].ndim >= 2)
        sw, se = ref["err"][:, 0].sum(), ref["err"][:, 1].sum()
        assert np.isclose(t["sqnr_db"], quant.sqnr_db(float(sw), float(se)), rtol=0.0, atol=1e-9, equal_nan=True), t["name"]
        assert t["max_error"] == ref["err"][:, 2].max(), t["name"]
        assert t["fp32_bytes"] == 4 * sd[t["name"]].size and t["int8_bytes"] == sd[t["name"]].size + 4 * t["rows"]
    assert "total" in str(rep) and "conv1.weight" in str(rep)


def test_update_follows_the_source_without_a_wait_or_an_allocation():
    model, sd = _golden_model("simple")
    wq = pkg.WeightQuant(model)
    x = _x(8)
    with torch.no_grad():
        before = wq.model(x).clone()
        versions = {k: p._version for k, p in wq.model.named_parameters()}
        model.conv2.weight.mul_(1.5)                               # in place: the same storage, other values
        model.fc.bias.add_(0.25)
        torch.cuda.synchronize()
        allocated = torch.cuda.memory_allocated()
        torch.cuda.set_sync_debug_mode("error")
        try:
            wq.update()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.cuda.memory_allocated() == allocated and wq.n_updates == 2 and len(wq._tables) == 1
        assert all(p._version > versions[k] for k, p in wq.model.named_parameters())
        after = wq.model(x)                                        # packed_weights() rebuilt
        judge = _reference_model("simple", _host_sd(model))
        assert _bits_equal(_np(after), _np(judge(x))) and not torch.equal(after, before)
        # another instance of the class is paired by name
        other = tt._model("simple", seed=77)
        wq.update(other)
        assert _bits_equal(_np(wq.model(x)), _np(_reference_model("simple", _host_sd(other))(x)))
        assert len(wq._tables) == 2


def test_weight_quant_around_an_averaged_model():
    model = tt._model("full")
    wa = pkg.WeightAverage(model, decay=0.5)
    wa.update()
    wq = pkg.WeightQuant(wa.model, bits=8)
    x = _x(8)
    with torch.no_grad():
        assert _bits_equal(_np(wq.model(x)), _np(_reference_model("full", _host_sd(wa.model))(x)))
        for p in model.parameters():
            p.mul_(1.25)
        wa.update()
        wq.update()
        assert _bits_equal(_np(wq.model(x)), _np(_reference_model("full", _host_sd(wa.model))(x)))


def test_evaluators_take_the_fake_quant_model():
    model, sd = _golden_model("simple")
    wq = pkg.WeightQuant(model)
    judge = _reference_model("simple", sd)
    x, y = tt._batch(24, 32, seed=9)
    loader = [(x[:16], y[:16]), (x[16:], y[16:])]
    assert pkg.evaluate_report(wq.model, loader) == pkg.evaluate_report(judge, loader)
    pcm = torch.from_numpy(pkg.synth.make_clips(0, 4)).to(DEV)
    with torch.no_grad():
        assert _bits_equal(_np(wq.model.forward_pcm(pcm)), _np(judge.forward_pcm(pcm)))
    dets = [pkg.StreamingDetector(m, n_mics=2, hop_samples=160) for m in (wq.model, judge)]
    hops = pcm[:2, :480].reshape(2, 3, 160)
    for j in range(3):
        for d in dets:
            d.step(hops[:, j].contiguous())
    for d in dets:
        d.detections()                                             # waits for the detector's stream
    assert _bits_equal(_np(dets[0].logits), _np(dets[1].logits)) and np.isfinite(_np(dets[0].prob)).all()
    for d in dets:
        d.close()


def test_package_round_trip_gives_the_bits_of_the_fake_quant_model(tmp_path):
    model, sd = _golden_model("full")
    wq = pkg.WeightQuant(model, bits=8)
    path = str(tmp_path / "quantized.pth")
    pkg.save_quantized_package(wq, path, best_val_accuracy=88.0, epoch=2)
    x = _x(8)
    with torch.no_grad():
        want = _np(wq.model(x))
        for device in ("cuda", "cpu"):
            fresh = pkg.WakewordModel().to(device)
            st = pkg.load_quantized_package(path, fresh)["quantized"]
            assert all(v.device.type == "cpu" and v.dtype == torch.int8 for v in st["q"].values())
            for (k, a), b in zip(fresh.named_parameters(), wq.model.parameters()):
                assert _bits_equal(_np(a), _np(b)), (device, k)
            if device == "cuda":
                assert _bits_equal(_np(fresh.eval()(x)), want)
        via_checkpoint = pkg.WakewordModel()
        pkg.model.load_checkpoint(via_checkpoint, path)            # model_state_dict: the dequantised float32 weights
        assert all(_bits_equal(_np(a), _np(b)) for a, b in zip(via_checkpoint.parameters(), wq.model.parameters()))
        # the state dict into another WeightQuant, on the GPU
        twin = pkg.WeightQuant(tt._model("full", seed=3), bits=4)
        twin.load_state_dict(wq.state_dict())
        assert twin.bits == 8 and _bits_equal(_np(twin.model(x)), want)


# ======================================================================================================================================
# trainer
# ======================================================================================================================================
B, T = 16, 8
NAMES = ("train_forward_into", "ce_loss_into", "soft_ce_loss_into", "train_backward_into", "grad_norm_launch", "adam_launch", "adam_average_launch",
         "weight_average_launch", "clip_metrics_update_into", "model_forward_into", "quantize_weights_launch")


def _record(monkeypatch, names=NAMES):
    calls = []
    for name in names:
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    return calls


def _validation_set():
    x, y = tt._batch(24, T, seed=31)
    return [(x[:16], y[:16]), (x[16:], y[16:])]


def test_evaluate_quant_follows_the_fake_quant_model(tmp_path):
    model = tt._model("simple")
    with pytest.raises(ValueError, match="quant"):
        pkg.WakewordTrainer(model, DEV, evaluate="quant")
    with pytest.raises(ValueError, match="evaluate"):
        pkg.WakewordTrainer(model, DEV, evaluate="int8")
    wq = pkg.WeightQuant(model, bits=4)
    trainer = pkg.WakewordTrainer(model, DEV, quant=wq, evaluate="quant", checkpoint_path=str(tmp_path / "best.pth"))
    val = _validation_set()
    torch.manual_seed(2)
    for round_ in range(2):                                        # the second round: re-quantised, so the packed weights were rebuilt
        model.train()
        for i in range(2):
            trainer.step(*tt._batch(B, T, seed=40 + 2 * round_ + i))
        got = trainer.validate(val)
        assert wq.n_updates == 2 + round_
        fresh = _reference_model("simple", _host_sd(model), bits=4)
        judge = pkg.WakewordTrainer(fresh, DEV)
        assert judge.validate(val) == got and judge.val_report == trainer.val_report
        for a, b in zip(wq.model.parameters(), fresh.parameters()):
            assert _bits_equal(_np(a), _np(b))
        assert not model.training and not wq.model.training
        raw = pkg.WakewordTrainer(model, DEV)
        assert raw.validate(val)[0] != got[0]                      # ... and it is not the float32 weights' loss
    # the checkpoint holds the integers of the weights it holds
    model.train()
    torch.manual_seed(3)
    xv = val[0][0][:1].repeat(8, 1, 1, 1)
    yv = torch.tensor([0, 1] * 4, device=DEV).view(8, 1)           # 50 % whatever the model says: the epoch is the best one so far
    trainer.train([tt._batch(B, T, seed=60)], [(xv, yv)], epochs=1)
    ckpt = torch.load(str(tmp_path / "best.pth"), weights_only=True)
    seven = ["epoch", "model_state_dict", "optimizer_state_dict", "val_acc", "train_acc", "train_loss", "val_loss"]
    assert sorted(ckpt) == sorted(seven + ["quant_state_dict"])
    st = ckpt["quant_state_dict"]
    assert st["bits"] == 4 and sorted(list(st["q"]) + list(st["float"])) == sorted(ckpt["model_state_dict"])
    for k, q in st["q"].items():
        ref = qref.quantize(_np(ckpt["model_state_dict"][k]), 4, True)
        assert _bits_equal(_np(q), ref["q"]) and _bits_equal(_np(st["scale"][k]), ref["scale"]), k
    # with a quantiser that validation does not follow, the checkpoint still gains its state, taken from the saved weights
    model2 = tt._model("simple", seed=8)
    wq2 = pkg.WeightQuant(model2)
    t2 = pkg.WakewordTrainer(model2, DEV, quant=wq2, checkpoint_path=str(tmp_path / "plain.pth"))
    torch.manual_seed(3)
    t2.train([tt._batch(B, T, seed=60)], [(xv, yv)], epochs=1)
    c2 = torch.load(str(tmp_path / "plain.pth"), weights_only=True)
    ref = qref.quantize(_np(c2["model_state_dict"]["fc.weight"]), 8, True)
    assert _bits_equal(_np(c2["quant_state_dict"]["q"]["fc.weight"]), ref["q"]) and wq2.n_updates == 2


def test_without_a_quantiser_every_native_call_is_what_it_was(monkeypatch):
    """quant=None: a step is forward, loss, backward, Adam and validate is loss and metrics per batch, nothing else; with a quantiser
    that validation follows, the steps are the same calls with the same bits and validate gains ONE launch in front."""
    x, y = tt._batch(B, T, seed=6)
    y = y.contiguous()
    val = _validation_set()
    runs = {}
    for with_quant in (False, True):
        model = tt._model("full")
        wq = pkg.WeightQuant(model) if with_quant else None
        trainer = pkg.WakewordTrainer(model, DEV, quant=wq, evaluate="quant" if with_quant else "model")
        model.train()
        torch.manual_seed(11)
        trainer.step(x, y)
        trainer.validate(val)
        model.train()
        torch.cuda.synchronize()
        calls = _record(monkeypatch)
        try:
            torch.cuda.set_sync_debug_mode("error")
            try:
                for _ in range(2):
                    trainer.step(x, y)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            n_step = len(calls)
            loss_acc = trainer.validate(val)
        finally:
            monkeypatch.undo()
        torch.cuda.synchronize()
        runs[with_quant] = (tt._state_of(model, trainer.optimizer), calls[:n_step], calls[n_step:], loss_acc)
    (plain, plain_step, plain_val, plain_result), (quantd, q_step, q_val, q_result) = runs[False], runs[True]
    assert plain_step == ["train_forward_into", "ce_loss_into", "train_backward_into", "adam_launch"] * 2
    assert plain_val == ["ce_loss_into", "clip_metrics_update_into"] * 2
    assert q_step == plain_step and q_val == ["quantize_weights_launch"] + plain_val
    for role in "pmv":
        for k in plain[role]:
            assert np.array_equal(plain[role][k].view(np.int32), quantd[role][k].view(np.int32)), (role, k)
    assert q_result != plain_result
