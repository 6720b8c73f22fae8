"""Quantisation-aware training without a GPU: the three C entry points are exported and bound with the header's
prototypes and refuse every bad argument before any HIP call, naming the field; the numpy reference (tests/qat_ref.py) obeys the
properties the rule promises; a clip="mse" package written around a CPU model loads back as q * scale bit for bit while clip="max" states
and packages keep exactly the keys they had; WeightQuant and the trainer refuse bad options before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import qat_ref as qat
import quant_ref as qref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import ops, quant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = nat.lib
HAS_GPU = torch.cuda.is_available()
ENTRIES = {"ww_quant_weights_clip_f32": nat.QuantClipTensor, "ww_quant_clip_search_f32": nat.QuantClipTensor, "ww_quant_ste_f32": nat.QuantSteTensor}


def _err():
    return (L.ww_last_error() or b"").decode()


# ---- the binding ----------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound_with_the_headers_prototypes():
    raw = open(os.path.join(ROOT, "include", "wakeword_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = C.CDLL(nat.LIB_PATH)
    for name, struct in ENTRIES.items():
        args = [C.POINTER(struct), C.c_int64, C.c_int, C.c_void_p]
        assert hasattr(lib, name) and nat.PROTOTYPES[name] == (C.c_int, args)
        assert getattr(L, name).argtypes == args and getattr(L, name).restype == C.c_int
        decl = re.sub(r"\s+", " ", re.search(rf"WW_API int {name}\((.*?)\);", text, flags=re.S).group(1))
        ctype = {nat.QuantClipTensor: "ww_quant_clip_tensor", nat.QuantSteTensor: "ww_quant_ste_tensor"}[struct]
        assert decl == f"const {ctype}* tensors_host, int64_t n_tensors, int bits, ww_stream_t stream"
    for ctype, struct, size in (("ww_quant_clip_tensor", nat.QuantClipTensor, 88), ("ww_quant_ste_tensor", nat.QuantSteTensor, 40)):
        body = re.search(rf"typedef struct {ctype} \{{(.*?)\}} {ctype};", text, flags=re.S).group(1)
        fields = [re.sub(r"\s+", " ", f.strip()) for f in body.split(";") if f.strip()]
        assert [n for n, _ in struct._fields_] == [f.split()[-1] for f in fields] and C.sizeof(struct) == size
        assert all(f.endswith(("rows", "cols")) == f.startswith("int64_t") for f in fields)          # pointers, then the two sizes
    assert re.search(r"#define WW_QUANT_CLIP_STEPS 48\b", raw) and nat.QUANT_CLIP_STEPS == 48 == qat.CLIP_STEPS
    # the shared fields of the clip struct are ww_quant_tensor's, in its order
    assert [n for n, _ in nat.QuantClipTensor._fields_][:6] == [n for n, _ in nat.QuantTensor._fields_][:6]


# ---- refusals: fake, never dereferenced addresses ---------------------------------------------------------------------------------------
def _clip_table(**kw):
    tab = (nat.QuantClipTensor * 17)()
    for k in range(17):
        e = tab[k]
        e.w, e.scale, e.q, e.deq, e.err, e.bad = (0x10000 + k * 0x1000, 0x20000 + k * 0x100, 0x30000 + k * 0x1000, 0x40000 + k * 0x1000,
                                                  0x50000 + k * 0x100, 0x60000 + k * 0x100)
        e.clip, e.sat, e.cand_err = 0x70000 + k * 0x100, 0x80000 + k * 0x100, 0x90000 + k * 0x1000
        e.rows, e.cols = 4, 9
    for name, v in kw.items():
        setattr(tab[int(name[-1])] if name[-1].isdigit() else tab[0], name.rstrip("0123456789"), v)
    return tab


def _ste_table(**kw):
    tab = (nat.QuantSteTensor * 17)()
    for k in range(17):
        e = tab[k]
        e.w, e.scale, e.g, e.rows, e.cols = 0x10000 + k * 0x1000, 0x20000 + k * 0x100, 0x40000 + k * 0x1000, 4, 9
    for name, v in kw.items():
        setattr(tab[int(name[-1])] if name[-1].isdigit() else tab[0], name.rstrip("0123456789"), v)
    return tab


def _call(entry, make, tab=None, n_tensors=4, bits=8, null_table=False):
    return getattr(L, entry)(None if null_table else (make() if tab is None else tab), n_tensors, bits, None)


COMMON = [(dict(null_table=True), "null"), (dict(n_tensors=0), "n_tensors"), (dict(n_tensors=17), "n_tensors"), (dict(n_tensors=-1), "n_tensors"),
          (dict(bits=1), "bits"), (dict(bits=9), "bits"), (dict(bits=0), "bits"), (dict(bits=-8), "bits")]
SHARED = [(dict(w=None), "tensors[0]"), (dict(scale=None), "tensors[0]"), (dict(w3=None), "tensors[3]"), (dict(scale2=None), "tensors[2]"),
          (dict(rows=0), "tensors[0].rows"), (dict(rows=-1), "tensors[0].rows"), (dict(cols=0), "tensors[0].cols"), (dict(cols1=-5), "tensors[1].cols"),
          (dict(rows=2 ** 31), "tensors[0].rows"), (dict(rows=2 ** 30, cols=2 ** 30), "rows x cols"), (dict(w=0x10002), "aligned"),
          (dict(scale=0x20001), "aligned")]
CLIP_ONLY = [(dict(deq=0x40002), "aligned"), (dict(bad=0x60002), "aligned"), (dict(err=0x50004), "err"), (dict(deq=0x10000), "overlap"),
             (dict(deq=0x10000 + 4 * 35), "overlap"), (dict(clip=None), "clip"), (dict(clip2=None), "tensors[2]"), (dict(sat=0x80002), "sat"),
             (dict(sat3=0x80301), "tensors[3]"), (dict(cand_err=0x90004), "cand_err"), (dict(cand_err1=0x91001), "tensors[1]")]
STE_ONLY = [(dict(g=None), "tensors[0]"), (dict(g3=None), "tensors[3]"), (dict(g=0x40002), "aligned"), (dict(g=0x10000), "overlap"),
            (dict(g=0x10000 + 4 * 35), "overlap"), (dict(g2=0x12000 - 4), "tensors[2]")]


@pytest.mark.parametrize("entry", ["ww_quant_weights_clip_f32", "ww_quant_clip_search_f32"])
@pytest.mark.parametrize("kw, word", COMMON + [(dict(tab=k), w) for k, w in SHARED + CLIP_ONLY])
def test_clip_entry_points_refuse_before_any_hip_call(entry, kw, word):
    kw = dict(kw, tab=_clip_table(**kw["tab"])) if "tab" in kw else kw
    assert _call(entry, _clip_table, **kw) == nat.WW_EINVAL and word in _err(), _err()


@pytest.mark.parametrize("kw, word", COMMON + [(dict(tab=k), w) for k, w in SHARED + STE_ONLY])
def test_ste_entry_point_refuses_before_any_hip_call(kw, word):
    kw = dict(kw, tab=_ste_table(**kw["tab"])) if "tab" in kw else kw
    assert _call("ww_quant_ste_f32", _ste_table, **kw) == nat.WW_EINVAL and word in _err(), _err()


def test_optional_outputs_may_be_null_and_the_device_check_comes_last():
    """Without a GPU a call whose arguments are all good ends at the device check and nowhere earlier."""
    if HAS_GPU:
        return                                                                     # fake addresses must never reach a kernel
    lean = dict(q=None, deq=None, err=None, bad=None, sat=None, cand_err=None)
    for tab in (_clip_table(), _clip_table(**lean), _clip_table(sat=None), _clip_table(cand_err=None), _clip_table(q=0x30001), _clip_table(clip=0x70003)):
        for entry in ("ww_quant_weights_clip_f32", "ww_quant_clip_search_f32"):
            for n, bits in ((1, 2), (16, 4), (16, 8)):
                assert _call(entry, _clip_table, tab=tab, n_tensors=n, bits=bits) == nat.WW_ENODEVICE, _err()
    for tab in (_ste_table(), _ste_table(g=0x10000 + 4 * 36)):
        for n, bits in ((1, 2), (16, 4), (16, 8)):
            assert _call("ww_quant_ste_f32", _ste_table, tab=tab, n_tensors=n, bits=bits) == nat.WW_ENODEVICE, _err()


# ---- the reference obeys its own properties --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [2, 3, 4, 8])
def test_reference_at_clip_zero_is_the_unclipped_rule_and_the_fractions_are_exact(bits):
    rng = np.random.default_rng(bits)
    w = (rng.standard_normal((7, 65)) * 10.0 ** rng.uniform(-30, 30, (7, 1))).astype(np.float32)
    w[3, 5], w[4, 7] = np.nan, -np.inf
    plain, zero = qref.quantize_rows(w, bits), qat.quantize_rows_clip(w, np.zeros(7, np.uint8), bits)
    for k in ("q", "scale", "deq", "bad", "err"):
        assert plain[k].tobytes() == zero[k].tobytes(), k
    assert not zero["sat"].any()
    f = qat.fractions(np.arange(300))
    assert f.dtype == np.float32 and f[0] == 1.0 and f[47] == np.float32(17 / 64) and np.all(f[47:] == f[47])
    assert np.array_equal(f[:48].astype(np.float64) * 64, 64 - np.arange(48))                      # exact
    clipped = qat.quantize_rows_clip(w, np.full(7, 47, np.uint8), bits)             # 17/64: the largest element lands at 3.76 qmax
    qmax = qref.qmax_of(bits)
    assert np.all(np.abs(clipped["q"].astype(int)) <= qmax) and clipped["sat"].sum() > 0
    moved = np.abs(np.rint(np.where(np.isfinite(w), w, 0) / clipped["scale"][:, None])) > qmax
    assert np.array_equal(clipped["sat"], moved.sum(axis=1)) and np.all(np.abs(clipped["q"][moved].astype(int)) == qmax)


def test_reference_search_finds_the_smallest_error_and_ties_keep_the_first():
    rng = np.random.default_rng(1234)
    w = (rng.standard_normal((5, 1024)) * 0.05).astype(np.float32)
    w[4] = 0.0
    s = qat.search_rows(w, 4)
    assert s["cand_err"].shape == (5, 48) and np.array_equal(s["clip"], s["cand_err"].argmin(axis=1)) and s["clip"][4] == 0
    assert np.array_equal(s["cand_err"][:, 0], qref.quantize_rows(w, 4)["err"][:, 1])
    assert np.all(s["clip"][:4] > 0) and np.all(s["cand_err"].min(axis=1)[:4] < s["cand_err"][:4, 0])   # Gaussian rows gain from a clip at 4 bits
    assert np.array_equal(s["scale"], qat.scales(w, s["clip"], 4))
    gain = 10 * np.log10(s["cand_err"][:4, 0].sum() / s["cand_err"][:4].min(axis=1).sum())
    assert 1.0 < gain < 3.0                                                                          # the 1.0 to 2.1 dB of the trial, with room
    one = qat.search_rows(np.array([[0.3], [-7.0]], np.float32), 4)
    assert not one["clip"].any()


def test_reference_ste_cuts_exactly_the_saturated_elements():
    w = np.array([[1.0, -1.0, 0.5, 0.74, 0.76, np.nan, np.inf, -0.0, 8.0]], np.float32)
    scale = np.array([0.1], np.float32)                                                               # qmax 7 at 4 bits: |w| > 0.75 saturates
    g = np.array([[np.nan, 2.0, 3.0, 4.0, -5.0, 6.0, 7.0, np.nan, -0.0]], np.float32)
    out = qat.ste_rows(w, scale, g, 4)
    assert out.view(np.int32).tolist() == [[0, 0] + g.view(np.int32)[0, 2:4].tolist() + [0] + g.view(np.int32)[0, 5:8].tolist() + [0]]
    assert np.array_equal(qat.ste_rows(w, scale, g, 8).view(np.int32), g.view(np.int32))             # qmax 127: nothing saturates


# ---- the export, around a CPU model ----------------------------------------------------------------------------------------------------
def _cpu_model(arch):
    model = pkg.SimpleWakewordModel() if arch == "simple" else pkg.WakewordModel()
    sd = pkg.synth.make_state_dict(arch, seed=1234)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model, sd


def _ref_state(sd, names, bits, clips):
    q, scale, flt = {}, {}, {}
    for k in names:
        if sd[k].ndim >= 2:
            out = qat.quantize_clip(sd[k], clips[k], bits, True)
            q[k], scale[k] = torch.from_numpy(out["q"]), torch.from_numpy(out["scale"])
        else:
            flt[k] = torch.from_numpy(sd[k].copy())
    return {"bits": bits, "per_channel": True, "quantize_bias": False, "q": q, "scale": scale, "float": flt,
            "clip": {k: torch.from_numpy(clips[k]) for k in q}}


def test_mse_package_round_trips_on_the_cpu(tmp_path):
    model, sd = _cpu_model("simple")
    wq = pkg.WeightQuant(model, bits=4, clip="mse")                                 # a CPU model: built, not calibrated
    assert wq.clip_mode == "mse" and wq.n_updates == 0 and wq.n_calibrations == 0 and list(wq.clip) == wq.quantized
    assert all(c.dtype == torch.uint8 and c.numel() == wq.scale[k].numel() for k, c in wq.clip.items())
    for call in (wq.update, wq.calibrate):
        with pytest.raises(RuntimeError, match="CPU"):
            call()
    names = [k for k, _ in model.named_parameters()]
    rng = np.random.default_rng(3)
    clips = {k: rng.integers(0, 48, sd[k].shape[0]).astype(np.uint8) for k in names if sd[k].ndim >= 2}
    wq.load_state_dict(_ref_state(sd, names, 4, clips))
    want = qat.fake_quant_clip_state_dict(sd, clips, 4)
    for k, p in wq.model.named_parameters():
        assert np.array_equal(p.numpy().view(np.int32), want[k].view(np.int32)), k
    state = wq.state_dict()
    assert sorted(state) == sorted(["bits", "per_channel", "quantize_bias", "q", "scale", "float", "clip"])
    assert all(np.array_equal(state["clip"][k].numpy(), clips[k]) for k in clips)
    path = str(tmp_path / "mse.pth")
    written = pkg.save_quantized_package(wq, path, best_val_accuracy=90.0, epoch=1, device="cpu")
    assert sorted(written["quantized"]) == sorted(state)
    fresh = pkg.SimpleWakewordModel()
    loaded = pkg.load_quantized_package(path, fresh)                                # q * scale alone
    for k, p in fresh.named_parameters():
        assert np.array_equal(p.detach().numpy().view(np.int32), want[k].view(np.int32)), k
    assert all(np.array_equal(loaded["quantized"]["clip"][k].numpy(), clips[k]) for k in clips)
    # a state without `clip` turns the object back into a "max" one, a state with it a "max" object into an "mse" one
    plain = pkg.WeightQuant(model, bits=8)
    plain.load_state_dict(state)
    assert plain.clip_mode == "mse" and plain.bits == 4 and all(np.array_equal(plain.clip[k].numpy(), clips[k]) for k in clips)
    del state["clip"]
    wq.load_state_dict(state)
    assert wq.clip_mode == "max" and not wq.clip and "clip" not in wq.state_dict()
    bad = _ref_state(sd, names, 4, clips)
    bad["clip"]["fc.weight"] = torch.zeros(3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="clip"):
        wq.load_state_dict(bad)


def test_max_states_and_packages_keep_exactly_their_keys(tmp_path):
    model, _ = _cpu_model("full")
    for wq in (pkg.WeightQuant(model), pkg.WeightQuant(model, clip="max")):
        assert wq.clip_mode == "max" and not wq.clip
        assert sorted(wq.state_dict()) == sorted(["bits", "per_channel", "quantize_bias", "q", "scale", "float"])
        written = pkg.save_quantized_package(wq, str(tmp_path / "max.pth"), device="cpu")
        assert sorted(written) == sorted(["model_state_dict", "model_config", "audio_config", "training_info", "classes", "quantized"])
        assert sorted(written["quantized"]) == sorted(["bits", "per_channel", "quantize_bias", "q", "scale", "float"])
        assert wq._stats.numel() == 32 * sum(s.numel() for s in wq.scale.values())                  # the report's buffer as it was
    mse = pkg.WeightQuant(model, clip="mse")
    assert mse._stats.numel() == 37 * sum(s.numel() for s in mse.scale.values())


# ---- refusals of the Python layers, before any device call -----------------------------------------------------------------------------
def test_weight_quant_and_ops_refuse_bad_clip_options():
    model = pkg.SimpleWakewordModel()
    for bad in ("MSE", "min", None, 0, True):
        with pytest.raises(ValueError, match="clip"):
            pkg.WeightQuant(model, clip=bad)
    assert ops.QUANT_CLIPS == ("max", "mse") and ops.check_quant_clip("mse") == "mse"
    w = torch.zeros(4, 9)
    for call in (lambda: ops.quantize_weights_clip([w], [torch.zeros(4, dtype=torch.uint8)]), lambda: ops.quant_clip_search([w]),
                 lambda: ops.quant_ste_([w], [torch.zeros(4)], [torch.zeros(4, 9)])):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()
    for call in (lambda: ops.quantize_weights_clip([w], [], bits=4), lambda: ops.quant_ste_([w], [], [])):
        with pytest.raises((ValueError, RuntimeError)):
            call()
    with pytest.raises(ValueError, match="bits"):
        ops.quant_clip_search([w], bits=9)
    with pytest.raises(ValueError, match="1..16"):
        ops.quant_clip_table([], [], [])
    with pytest.raises(ValueError, match="1..16"):
        ops.quant_ste_table([], [], [])
    assert ops.quantize_weights_clip([], []) == [] and ops.quant_clip_search([]) == []
    assert quant.clip_fractions(torch.tensor([0, 1, 47, 48, 255], dtype=torch.uint8)).tolist() == [1.0, 63 / 64, 17 / 64, 17 / 64, 17 / 64]


def test_trainer_refuses_bad_qat_options_before_any_device_call():
    model = pkg.SimpleWakewordModel()                                              # on the CPU: the refusals below come first
    wq = pkg.WeightQuant(model, bits=4, clip="mse")
    with pytest.raises(ValueError, match="qat=True needs a quantiser"):
        pkg.WakewordTrainer(model, "cpu", qat=True)
    with pytest.raises(TypeError, match="qat"):
        pkg.WakewordTrainer(model, "cpu", quant=wq, qat=1)
    for bad in ("step", 0, -3, 2.0, True):
        with pytest.raises(ValueError, match="qat_calibrate"):
            pkg.WakewordTrainer(model, "cpu", quant=wq, qat=True, qat_calibrate=bad)
    with pytest.raises(NotImplementedError, match="select"):
        pkg.WakewordTrainer(model, "cpu", quant=wq, qat=True, select=pkg.HardSelect(4))
    with pytest.raises(ValueError, match="another model"):
        pkg.WakewordTrainer(model, "cpu", quant=pkg.WeightQuant(pkg.SimpleWakewordModel()), qat=True)
    with pytest.raises(ValueError, match="another model"):
        pkg.WakewordTrainer(model, "cpu", quant=pkg.WeightQuant(pkg.WeightAverage(model).model), qat=True)
    with pytest.raises(NotImplementedError, match="quantize_bias"):
        pkg.WakewordTrainer(model, "cpu", quant=pkg.WeightQuant(model, clip="mse", quantize_bias=True), qat=True)
    if not HAS_GPU:
        for kw in (dict(qat=True), dict(qat=True, qat_calibrate=5), dict(qat=True, qat_calibrate=None), dict(qat=False, qat_calibrate=None),
                   dict(qat=True, evaluate="quant")):
            with pytest.raises(TypeError, match="CPU"):                            # good options: only the device is missing
                pkg.WakewordTrainer(model, "cpu", quant=wq, **kw)
        with pytest.raises(TypeError, match="CPU"):
            pkg.WakewordTrainer(model, "cpu", quant=pkg.WeightQuant(model, quantize_bias=True), qat=True)
