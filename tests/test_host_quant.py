"""Weight quantisation without a GPU: the C entry point is exported and bound with the header's prototype and
refuses every bad argument before any HIP call, naming the field; the numpy reference (tests/quant_ref.py) obeys the properties the rule
promises; a quantised package written around a CPU model loads back as q * scale bit for bit and loads with load_checkpoint too; WeightQuant
and the trainer refuse bad options before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import quant_ref as qref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import ops, quant
from wakeword_jupyterlab_amd.model import load_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = nat.lib
HAS_GPU = torch.cuda.is_available()


def _err():
    return (L.ww_last_error() or b"").decode()


# ---- the binding ----------------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_bound_with_the_headers_prototype():
    assert L.ww_abi_version() == 4 == nat.ABI_VERSION
    args = [C.POINTER(nat.QuantTensor), C.c_int64, C.c_int, C.c_void_p]
    assert hasattr(C.CDLL(nat.LIB_PATH), "ww_quant_weights_f32") and nat.PROTOTYPES["ww_quant_weights_f32"] == (C.c_int, args)
    assert L.ww_quant_weights_f32.argtypes == args and L.ww_quant_weights_f32.restype == C.c_int
    raw = open(os.path.join(ROOT, "include", "wakeword_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    decl = re.sub(r"\s+", " ", re.search(r"WW_API int ww_quant_weights_f32\((.*?)\);", text, flags=re.S).group(1))
    assert decl == "const ww_quant_tensor* tensors_host, int64_t n_tensors, int bits, ww_stream_t stream"
    # the struct, field for field: six pointers, rows, cols -- 64 bytes
    body = re.search(r"typedef struct ww_quant_tensor \{(.*?)\} ww_quant_tensor;", text, flags=re.S).group(1)
    fields = [re.sub(r"\s+", " ", f.strip()) for f in body.split(";") if f.strip()]
    assert fields == ["const float* w", "float* scale", "int8_t* q", "float* deq", "double* err", "int32_t* bad", "int64_t rows", "int64_t cols"]
    assert [n for n, _ in nat.QuantTensor._fields_] == [f.split()[-1] for f in fields] and C.sizeof(nat.QuantTensor) == 64
    assert re.search(r"#define WW_QUANT_MAX_TENSORS 16\b", raw) and nat.QUANT_MAX_TENSORS == 16


# ---- refusals: fake, never dereferenced addresses ---------------------------------------------------------------------------------------
def _table(**kw):
    tab = (nat.QuantTensor * 17)()
    for k in range(17):
        e = tab[k]
        e.w, e.scale, e.q, e.deq, e.err, e.bad = (0x10000 + k * 0x1000, 0x20000 + k * 0x100, 0x30000 + k * 0x1000, 0x40000 + k * 0x1000,
                                                  0x50000 + k * 0x100, 0x60000 + k * 0x100)
        e.rows, e.cols = 4, 9
    for name, v in kw.items():
        setattr(tab[int(name[-1])] if name[-1].isdigit() else tab[0], name.rstrip("0123456789"), v)
    return tab


def _call(tab=None, n_tensors=4, bits=8, null_table=False):
    return L.ww_quant_weights_f32(None if null_table else (_table() if tab is None else tab), n_tensors, bits, None)


@pytest.mark.parametrize("kw, word", [
    (dict(null_table=True), "null"), (dict(n_tensors=0), "n_tensors"), (dict(n_tensors=17), "n_tensors"), (dict(n_tensors=-1), "n_tensors"),
    (dict(bits=1), "bits"), (dict(bits=9), "bits"), (dict(bits=0), "bits"), (dict(bits=-8), "bits"),
    (dict(tab=_table(w=None)), "tensors[0]"), (dict(tab=_table(scale=None)), "tensors[0]"), (dict(tab=_table(w3=None)), "tensors[3]"),
    (dict(tab=_table(scale2=None)), "tensors[2]"),
    (dict(tab=_table(rows=0)), "tensors[0].rows"), (dict(tab=_table(rows=-1)), "tensors[0].rows"), (dict(tab=_table(cols=0)), "tensors[0].cols"),
    (dict(tab=_table(cols1=-5)), "tensors[1].cols"), (dict(tab=_table(rows=2 ** 31)), "tensors[0].rows"),
    (dict(tab=_table(rows=2 ** 30, cols=2 ** 30)), "rows x cols"),
    (dict(tab=_table(w=0x10002)), "aligned"), (dict(tab=_table(scale=0x20001)), "aligned"), (dict(tab=_table(deq=0x40002)), "aligned"),
    (dict(tab=_table(bad=0x60002)), "aligned"), (dict(tab=_table(err=0x50004)), "err"),
    (dict(tab=_table(deq=0x10000)), "overlap"), (dict(tab=_table(deq=0x10000 + 4 * 35)), "overlap"),
])
def test_entry_point_refuses_before_any_hip_call(kw, word):
    assert _call(**kw) == nat.WW_EINVAL and word in _err(), _err()


def test_optional_outputs_may_be_null_and_the_device_check_comes_last():
    """Without a GPU a call whose arguments are all good ends at the device check and nowhere earlier: q, deq, err, bad may be NULL, a q
    may sit at any byte address, deq may touch another tensor's w... the entry is refused for the missing device alone."""
    if HAS_GPU:
        return                                                                     # fake addresses must never reach a kernel
    for tab in (_table(), _table(q=None), _table(deq=None), _table(err=None), _table(bad=None), _table(q=None, deq=None, err=None, bad=None),
                _table(q=0x30001), _table(deq=0x10000 + 4 * 36)):
        for n in (1, 16):
            for bits in (2, 4, 8):
                assert _call(tab=tab, n_tensors=n, bits=bits) == nat.WW_ENODEVICE, _err()


# ---- the reference obeys its own properties --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [2, 3, 4, 8])
def test_reference_stays_in_range_and_uses_the_whole_range(bits):
    rng = np.random.default_rng(bits)
    w = (rng.standard_normal((7, 65)) * 10.0 ** rng.uniform(-30, 30, (7, 1))).astype(np.float32)
    out = qref.quantize_rows(w, bits)
    qmax = qref.qmax_of(bits)
    assert out["q"].dtype == np.int8 and int(np.abs(out["q"].astype(int)).max()) == qmax            # every row's largest element is +-qmax
    assert np.all(np.abs(out["q"].astype(int)).max(axis=1) == qmax)
    # half a step, plus the two roundings at a ratio of up to 127: 2 x 127 x 2^-24 < 2^-16 of a step
    assert np.all(np.abs(w.astype(np.float64) - out["deq"]) <= (0.5 + 2.0 ** -16) * out["scale"].astype(np.float64)[:, None])
    assert np.all(out["bad"] == 0) and np.all(out["err"][:, 2] == np.abs(w.astype(np.float64) - out["deq"]).max(axis=1))


def test_reference_ties_go_to_even_and_zero_rows_get_the_floor():
    row = np.array([[127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5, -0.0]], np.float32)             # scale is exactly 1
    out = qref.quantize_rows(row, 8)
    assert out["scale"][0] == 1.0 and out["q"][0].tolist() == [127, 0, 2, 2, 0, -2, -2, 4, 0]
    assert not np.signbit(out["deq"][0, -1]) and not np.signbit(out["deq"][0, 1])                   # -0.0 and -0.5 dequantise to +0.0
    zero = qref.quantize_rows(np.zeros((2, 9), np.float32), 8)
    assert np.all(zero["scale"] == np.float32(2.0 ** -126)) and not zero["q"].any() and not zero["deq"].any() and not zero["err"].any()
    tiny = qref.quantize_rows(np.full((1, 4), 2.0 ** -140, np.float32), 8)                          # amax / 127 is below the floor
    assert tiny["scale"][0] == np.float32(2.0 ** -126) and not tiny["q"].any()
    sub = qref.quantize_rows(np.array([[2.0 ** -127, -(2.0 ** -128), 2.0 ** -149]], np.float32), 8) # a subnormal amax that still counts
    assert sub["scale"][0] == np.float32(2.0 ** -126) and sub["q"][0].tolist() == [0, 0, 0]         # 0.5 -> 0 (even), -0.25, 2^-23
    big = qref.quantize_rows(np.array([[3e38, -3e38, 1e38, 0.0]], np.float32), 8)
    assert np.isfinite(big["deq"]).all() and big["q"][0].tolist()[:2] == [127, -127]


def test_reference_counts_non_finite_elements_and_leaves_them_out():
    w = np.array([[64.0, np.nan, -127.0, np.inf, 16.25, -np.inf], [np.nan] * 6], np.float32)          # amax 127: the scale is exactly 1
    out = qref.quantize_rows(w, 8)
    assert out["bad"].tolist() == [3, 6] and out["scale"][0] == 1.0 and out["scale"][1] == np.float32(2.0 ** -126)
    assert out["q"][0].tolist() == [64, 0, -127, 0, 16, 0] and not out["q"][1].any() and not out["deq"][1].any()
    assert np.isfinite(out["err"]).all() and out["err"][1].tolist() == [0.0, 0.0, 0.0] and out["err"][0].tolist() == [64.0 ** 2 + 127.0 ** 2 + 16.25 ** 2, 0.0625, 0.25]


# ---- the export, around a CPU model ----------------------------------------------------------------------------------------------------
def _cpu_model(arch):
    model = pkg.SimpleWakewordModel() if arch == "simple" else pkg.WakewordModel()
    sd = pkg.synth.make_state_dict(arch, seed=1234)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model, sd


def _ref_state(sd, names, bits, per_channel, quantize_bias):
    """quant.WeightQuant.state_dict() as the reference computes it."""
    q, scale, flt = {}, {}, {}
    for k in names:
        v = sd[k]
        if v.ndim >= 2 or quantize_bias:
            out = qref.quantize(v, bits, per_channel and v.ndim >= 2)
            q[k], scale[k] = torch.from_numpy(out["q"]), torch.from_numpy(out["scale"])
        else:
            flt[k] = torch.from_numpy(v.copy())
    return {"bits": bits, "per_channel": per_channel, "quantize_bias": quantize_bias, "q": q, "scale": scale, "float": flt}


@pytest.mark.parametrize("arch, bits, per_channel, quantize_bias", [("simple", 8, True, False), ("full", 4, True, True), ("simple", 6, False, False)])
def test_package_round_trip_on_the_cpu(tmp_path, arch, bits, per_channel, quantize_bias):
    model, sd = _cpu_model(arch)
    wq = pkg.WeightQuant(model, bits=8, per_channel=True)                         # a CPU model: built, not quantised
    assert wq.n_updates == 0 and type(wq.model) is type(model) and not wq.model.training and model.training
    assert all(not p.requires_grad for p in wq.model.parameters())
    with pytest.raises(RuntimeError, match="CPU"):
        wq.update()
    names = [k for k, _ in model.named_parameters()]
    wq.load_state_dict(_ref_state(sd, names, bits, per_channel, quantize_bias))  # ... the options travel with the state
    assert (wq.bits, wq.per_channel, wq.quantize_bias) == (bits, per_channel, quantize_bias)
    want = qref.fake_quant_state_dict(sd, bits, per_channel, quantize_bias)
    for k, p in wq.model.named_parameters():
        assert np.array_equal(p.numpy().view(np.int32), want[k].view(np.int32)), k
    path = str(tmp_path / "quantized.pth")
    written = pkg.save_quantized_package(wq, path, best_val_accuracy=91.5, epoch=3, device="cpu")
    assert sorted(written) == sorted(["model_state_dict", "model_config", "audio_config", "training_info", "classes", "quantized"])
    # q * scale alone, bit for bit, into a fresh model ...
    fresh = type(model)()
    loaded = pkg.load_quantized_package(path, fresh)
    for k, p in fresh.named_parameters():
        assert np.array_equal(p.detach().numpy().view(np.int32), want[k].view(np.int32)), k
    st = loaded["quantized"]
    assert (st["bits"], st["per_channel"], st["quantize_bias"]) == (bits, per_channel, quantize_bias)
    assert all(v.dtype == torch.int8 for v in st["q"].values()) and all(v.dtype == torch.float32 for v in st["scale"].values())
    assert int(max(v.abs().max() for v in st["q"].values())) == qref.qmax_of(bits)
    assert sorted(list(st["q"]) + list(st["float"])) == sorted(names)
    # ... and the same file through load_checkpoint: the dequantised float32 weights
    other = type(model)()
    ckpt = load_checkpoint(other, path)
    assert ckpt["training_info"]["best_val_accuracy"] == 91.5 and ckpt["classes"] == ["negative", "wakeword"]
    for k, p in other.named_parameters():
        assert np.array_equal(p.detach().numpy().view(np.int32), want[k].view(np.int32)), k
    # a plain deployment package has no integers to load
    from wakeword_jupyterlab_amd.model import save_deployment_package
    save_deployment_package(model, str(tmp_path / "plain.pth"))
    with pytest.raises(ValueError, match="quantized"):
        pkg.load_quantized_package(str(tmp_path / "plain.pth"), fresh)


def test_dequantize_is_one_float32_multiplication():
    q = torch.tensor([[127, -127, 3], [1, 0, -2]], dtype=torch.int8)
    s = torch.tensor([0.1, 3.0e-39], dtype=torch.float32)                          # a subnormal scale stays one
    got = quant.dequantize(q, s).numpy()
    want = q.numpy().astype(np.float32) * s.numpy()[:, None]
    assert np.array_equal(got.view(np.int32), want.view(np.int32)) and got[1, 0] != 0.0
    assert quant.dequantize(q, torch.tensor([0.5])).tolist() == [[63.5, -63.5, 1.5], [0.5, 0.0, -1.0]]
    with pytest.raises(ValueError):
        quant.dequantize(q, torch.ones(3))
    with pytest.raises(TypeError):
        quant.dequantize(q.float(), s)


# ---- refusals of the Python layers, before any device call -----------------------------------------------------------------------------
def test_lazy_exports_and_weight_quant_refusals():
    assert pkg.WeightQuant is quant.WeightQuant and pkg.quant is quant and pkg.QuantReport is quant.QuantReport
    assert pkg.save_quantized_package is quant.save_quantized_package and pkg.load_quantized_package is quant.load_quantized_package
    model = pkg.SimpleWakewordModel()
    for bad in (dict(bits=1), dict(bits=9), dict(bits=8.0), dict(bits=True), dict(bits="8")):
        with pytest.raises(ValueError, match="bits"):
            pkg.WeightQuant(model, **bad)
    for bad in (dict(per_channel=1), dict(per_channel="row"), dict(quantize_bias=None)):
        with pytest.raises(TypeError):
            pkg.WeightQuant(model, **bad)
    for bad in (torch.nn.Linear(3, 2), [torch.zeros(3)], None):
        with pytest.raises(TypeError, match="WeightQuant"):
            pkg.WeightQuant(bad)
    with pytest.raises(TypeError):
        pkg.save_quantized_package(model, "unused.pth")
    wq = pkg.WeightQuant(model, bits=4, per_channel=False, quantize_bias=True)
    assert (wq.bits, wq.per_channel, wq.quantize_bias) == (4, False, True) and wq.quantized == [k for k, _ in model.named_parameters()] and not wq.kept
    assert all(s.numel() == 1 for s in wq.scale.values())
    rows = pkg.WeightQuant(model)
    assert rows.kept == [k for k, p in model.named_parameters() if p.dim() == 1]
    assert rows.scale["conv1.weight"].numel() == 32 and rows.scale["lstm.weight_ih_l0"].numel() == 1024 and rows.scale["fc.weight"].numel() == 2
    assert rows.q["conv2.weight"].shape == (64, 32, 3, 3) and rows.q["conv2.weight"].dtype == torch.int8
    with pytest.raises(ValueError, match="names"):
        rows.update(pkg.WakewordModel())


def test_ops_wrappers_refuse_before_any_device_call():
    w = torch.zeros(4, 9)
    for call in (lambda: ops.quantize_weights([w], bits=1), lambda: ops.quantize_weights([w], bits=9), lambda: ops.quantize_weights([w], bits=4.0)):
        with pytest.raises(ValueError, match="bits"):
            call()
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        ops.quantize_weights([w])
    with pytest.raises(TypeError):
        ops.quantize_weights([np.zeros((4, 9), np.float32)])
    with pytest.raises(ValueError, match="per_channel"):
        ops.quantize_weights([w, w], per_channel=[True])
    with pytest.raises(ValueError, match="1..16"):
        ops.quant_table([], [])
    assert ops.quantize_weights([]) == []
    assert ops.quant_groups(torch.zeros(64, 32, 3, 3)) == (64, 288) and ops.quant_groups(torch.zeros(64, 32, 3, 3), False) == (1, 18432)
    assert ops.quant_groups(torch.zeros(7)) == (1, 7)


def test_trainer_refuses_bad_quant_options_before_any_device_call():
    model = pkg.SimpleWakewordModel()                                              # on the CPU: the refusals below come first
    with pytest.raises(ValueError, match="quant"):
        pkg.WakewordTrainer(model, "cpu", evaluate="quant")
    with pytest.raises(TypeError, match="WeightQuant"):
        pkg.WakewordTrainer(model, "cpu", quant=object())
    with pytest.raises(TypeError, match="WeightQuant"):
        pkg.WakewordTrainer(model, "cpu", quant=pkg.WeightAverage(model), evaluate="quant")
    if not HAS_GPU:
        with pytest.raises(TypeError, match="CPU"):                                # good options: only the device is missing
            pkg.WakewordTrainer(model, "cpu", quant=pkg.WeightQuant(model), evaluate="quant")


def test_report_arithmetic():
    assert quant.sqnr_db(100.0, 1.0) == 20.0 and quant.sqnr_db(1.0, 0.0) == float("inf") and quant.sqnr_db(0.0, 0.0) != quant.sqnr_db(0.0, 0.0)
    tensors = [dict(name="a", shape=(2, 3), rows=2, cols=3, fp32_bytes=24, int8_bytes=14, sum_w2=3.0, sum_err2=0.03, sqnr_db=20.0, max_error=0.1,
                    nonfinite=0),
               dict(name="b", shape=(4,), rows=1, cols=4, fp32_bytes=16, int8_bytes=8, sum_w2=1.0, sum_err2=0.01, sqnr_db=20.0, max_error=0.2,
                    nonfinite=2)]
    rep = quant.QuantReport(8, True, tensors, float_bytes=12)
    t = rep.totals
    assert (t["tensors"], t["rows"], t["fp32_bytes"], t["int8_bytes"], t["float_bytes"], t["max_error"], t["nonfinite"]) == (2, 3, 40, 22, 12, 0.2, 2)
    assert abs(t["sqnr_db"] - 20.0) < 1e-12
    text = str(rep)
    assert "int8" in text and "a" in text and "2x3" in text and "total" in text and "12 bytes" in text
