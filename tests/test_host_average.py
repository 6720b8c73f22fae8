"""WeightAverage without a GPU: the two C entry points are exported and bound with the header's prototypes and
refuse every bad argument before any HIP call, naming the field; the schedule `average.update_weight` drives a float64 recursion to what
torch.optim.swa_utils.AveragedModel computes in float64, for EMA and for SWA; the warmup values are the closed form; the averaged
weights move between WeightAverage and AveragedModel in both directions."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

import average_ref as aref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat
from wakeword_jupyterlab_amd import average

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = nat.lib
HAS_GPU = torch.cuda.is_available()


def _err():
    return (L.ww_last_error() or b"").decode()


def test_both_symbols_are_exported_and_bound_and_the_abi_stays_4():
    assert L.ww_abi_version() == 4 == nat.ABI_VERSION
    lib = C.CDLL(nat.LIB_PATH)
    want = {"ww_adam_avg_step_f32": [C.POINTER(nat.AdamTensor), C.POINTER(C.c_void_p), C.c_int64] + [C.c_double] * 5 +
                                    [C.c_int64, C.c_void_p, C.c_double, C.c_void_p],
            "ww_weight_average_f32": [C.POINTER(nat.AdamTensor), C.POINTER(C.c_void_p), C.c_int64, C.c_double, C.c_void_p]}
    for name, args in want.items():
        assert hasattr(lib, name) and nat.PROTOTYPES[name] == (C.c_int, args)
        assert getattr(L, name).argtypes == args and getattr(L, name).restype == C.c_int
    # the header's declarations, parameter for parameter
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wakeword_amd.h")).read(), flags=re.S)
    flat = lambda name: re.sub(r"\s+", " ", re.search(rf"WW_API int {name}\((.*?)\);", text, flags=re.S).group(1))     # noqa: E731
    assert flat("ww_adam_avg_step_f32") == ("const ww_adam_tensor* tensors_host, float* const* avg_host, int64_t n_tensors, double lr, double beta1, "
                                            "double beta2, double eps, double weight_decay, int64_t step, const float* grad_scale_dev, "
                                            "double avg_weight, ww_stream_t stream")
    assert flat("ww_weight_average_f32") == ("const ww_adam_tensor* tensors_host, float* const* avg_host, int64_t n_tensors, double avg_weight, "
                                             "ww_stream_t stream")
    assert C.sizeof(nat.AdamTensor) == 40
    assert L.ww_adam_step_f32.argtypes == [C.POINTER(nat.AdamTensor), C.c_int64] + [C.c_double] * 5 + [C.c_int64, C.c_void_p, C.c_void_p]


# ---- refusals: fake, never dereferenced addresses, as tests/test_host_trainer.py's _table -----------------------------------------
def _table(**kw):
    tab = (nat.AdamTensor * 17)()
    for k in range(17):
        tab[k].p, tab[k].g, tab[k].m, tab[k].v, tab[k].n = 0x10000 + k * 0x100, 0x20000 + k * 0x100, 0x30000 + k * 0x100, 0x40000 + k * 0x100, 8
    for k, v in kw.items():
        setattr(tab[0], k, v)
    return tab


def _avgs(**kw):
    """17 average pointers at 0x50000 + k 0x100; `a3=0x123` replaces entry 3."""
    arr = (C.c_void_p * 17)(*[0x50000 + k * 0x100 for k in range(17)])
    for k, v in kw.items():
        arr[int(k[1:])] = v
    return arr


def _fused(tab=None, avgs=None, n_tensors=4, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, step=1, w=0.1, null_avgs=False):
    return L.ww_adam_avg_step_f32(_table() if tab is None else tab, None if null_avgs else (_avgs() if avgs is None else avgs), n_tensors,
                                  lr, beta1, beta2, eps, wd, step, None, w, None)


def _alone(tab=None, avgs=None, n_tensors=4, w=0.1, null_avgs=False):
    return L.ww_weight_average_f32(_table() if tab is None else tab, None if null_avgs else (_avgs() if avgs is None else avgs), n_tensors, w, None)


AVERAGE_REFUSALS = [
    (dict(w=float("nan")), "avg_weight"), (dict(w=-0.001), "avg_weight"), (dict(w=1.001), "avg_weight"), (dict(w=float("inf")), "avg_weight"),
    (dict(null_avgs=True), "avg_host"), (dict(avgs=_avgs(a0=None)), "avg_host[0]"), (dict(avgs=_avgs(a3=None)), "avg_host[3]"),
    (dict(avgs=_avgs(a2=0x50202)), "avg_host[2]"), (dict(avgs=_avgs(a2=0x50201)), "aligned"),
    (dict(avgs=_avgs(a1=0x50000)), "overlap"), (dict(avgs=_avgs(a1=0x5001c)), "overlap"),           # another average: equal, and by one float
    (dict(avgs=_avgs(a1=0x10200)), "overlap"), (dict(avgs=_avgs(a3=0x1001c)), "overlap"),           # a p range, of another entry too
]


@pytest.mark.parametrize("kw, word", [
    # everything ww_adam_step_f32 checks ...
    (dict(n_tensors=0), "n_tensors"), (dict(n_tensors=17), "n_tensors"), (dict(lr=float("nan")), "lr"), (dict(lr=-1e-3), "lr"),
    (dict(beta1=1.0), "beta1"), (dict(beta2=float("nan")), "beta2"), (dict(eps=0.0), "eps"), (dict(wd=-1e-5), "weight_decay"),
    (dict(step=0), "step"), (dict(tab=_table(n=0)), "tensors[0].n"), (dict(tab=_table(p=None)), "null"), (dict(tab=_table(g=None)), "null"),
    (dict(tab=_table(m=None)), "null"), (dict(tab=_table(v=None)), "null"), (dict(tab=_table(p=0x10002)), "aligned"),
    (dict(tab=_table(m=0x10100)), "overlap"), (dict(tab=_table(v=0x3001c)), "overlap"),
    # ... and the averages: also against the m, v and g ranges of the table
    *AVERAGE_REFUSALS,
    (dict(avgs=_avgs(a0=0x30100)), "overlap"), (dict(avgs=_avgs(a0=0x4011c)), "overlap"), (dict(avgs=_avgs(a2=0x20000)), "overlap"),
    (dict(avgs=_avgs(a2=0x2031c)), "overlap"),
])
def test_fused_entry_refuses_before_any_hip_call(kw, word):
    assert _fused(**kw) == nat.WW_EINVAL and word in _err(), _err()


@pytest.mark.parametrize("kw, word", [
    (dict(n_tensors=0), "n_tensors"), (dict(n_tensors=17), "n_tensors"), (dict(tab=_table(n=0)), "tensors[0].n"), (dict(tab=_table(n=-3)), "tensors[0].n"),
    (dict(tab=_table(p=None)), "null"), (dict(tab=_table(p=0x10002)), "aligned"),
    *AVERAGE_REFUSALS,
])
def test_stand_alone_entry_refuses_before_any_hip_call(kw, word):
    assert _alone(**kw) == nat.WW_EINVAL and word in _err(), _err()


def test_null_tables_and_the_device_check_comes_last():
    assert L.ww_adam_avg_step_f32(None, _avgs(), 2, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, 0.1, None) == nat.WW_EINVAL and "null" in _err()
    assert L.ww_weight_average_f32(None, _avgs(), 2, 0.1, None) == nat.WW_EINVAL and "null" in _err()
    assert L.ww_adam_avg_step_f32(_table(), _avgs(), 2, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0x1002, 0.1, None) == nat.WW_EINVAL and "grad_scale_dev" in _err()
    if not HAS_GPU:
        shared = _table()
        shared[1].g = shared[0].g                                  # two entries may share a gradient, as in ww_adam_step_f32
        for w in (0.0, 0.1, 0.5, 1.0):
            assert _fused(tab=shared, n_tensors=16, w=w) == nat.WW_ENODEVICE
            assert _alone(n_tensors=16, w=w) == nat.WW_ENODEVICE
        # the stand-alone entry reads p and n only: g, m and v may be anything, an average may even lie on them
        assert _alone(tab=_table(g=None, m=0x3, v=0x10000), avgs=_avgs(a0=0x20000)) == nat.WW_ENODEVICE


# ---- the schedule ------------------------------------------------------------------------------------------------------------------
def test_first_update_copies_and_bad_arguments_are_refused():
    for mode in ("ema", "swa"):
        assert average.update_weight(0, mode, 0.9, True) == 1.0 == average.update_weight(0, mode, 0.5, False)
    assert average.update_weight(3, "swa") == 0.25 and average.update_weight(1, "ema", 0.999) == 1.0 - 0.999
    for bad in (dict(n=-1), dict(n=1.5), dict(n=1, mode="mean"), dict(n=1, decay=1.5), dict(n=1, decay=-0.1)):
        with pytest.raises(ValueError):
            average.update_weight(**bad)


def test_warmup_values_are_the_closed_form():
    for decay in (0.9, 0.999):
        for n in range(21):
            want = 1.0 if n == 0 else 1.0 - min(decay, (1.0 + n) / (10.0 + n))
            assert average.update_weight(n, "ema", decay, warmup=True) == want
    assert average.update_weight(1, "ema", 0.999, True) == 1.0 - 2.0 / 11.0 and average.update_weight(20, "ema", 0.6, True) == 1.0 - 0.6


@pytest.mark.parametrize("mode", ["ema", "swa"])
def test_float64_recursion_equals_torch_averaged_model(mode):
    """12 updates of small random float64 tensors: the recursion of tests/average_ref.py driven by update_weight against AveragedModel with
    get_ema_multi_avg_fn(0.9), and against the default (SWA) AveragedModel, to 1e-14 relative."""
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Linear(7, 3)).double()
    am = AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(0.9)) if mode == "ema" else AveragedModel(net)
    rng = np.random.default_rng(11)
    snaps = []
    for _ in range(12):
        with torch.no_grad():
            for p in net.parameters():
                p.copy_(torch.from_numpy(rng.standard_normal(tuple(p.shape))))
        am.update_parameters(net)
        snaps.append(np.concatenate([p.detach().numpy().reshape(-1) for p in net.parameters()]))
    ours = aref.recursion(snaps, [average.update_weight(n, mode, 0.9) for n in range(12)])
    theirs = np.concatenate([p.detach().numpy().reshape(-1) for p in am.module.parameters()])
    assert int(am.n_averaged) == 12
    assert float(np.abs(ours - theirs).max()) <= 1e-14 * float(np.abs(theirs).max())
    if mode == "swa":
        assert float(np.abs(ours - np.mean(snaps, axis=0)).max()) <= 1e-14 * float(np.abs(theirs).max())


# ---- the class, as far as it goes without a GPU -------------------------------------------------------------------------------------
def test_lazy_exports_and_constructor_refusals():
    assert pkg.WeightAverage is average.WeightAverage and pkg.average is average
    model = pkg.SimpleWakewordModel()
    for bad in (dict(mode="mean"), dict(every="batch"), dict(decay=1.5), dict(start=-1), dict(start=0.5)):
        with pytest.raises(ValueError):
            pkg.WeightAverage(model, **bad)
    with pytest.raises(TypeError):
        pkg.WeightAverage([torch.zeros(3)])
    wa = pkg.WeightAverage(model)
    assert (wa.mode, wa.decay, wa.warmup, wa.every, wa.start, wa.n_averaged) == ("ema", 0.999, False, "step", 0, 0)
    assert type(wa.model) is type(model) and not wa.model.training and model.training
    assert all(not p.requires_grad and p.grad is None for p in wa.model.parameters())
    assert all(torch.equal(a, p) and a.data_ptr() != p.data_ptr() for a, p in zip(wa.model.parameters(), model.parameters()))
    assert wa.average_of(model.fc.weight) is wa.model.fc.weight and wa.average_of(torch.nn.Parameter(torch.zeros(1))) is None
    assert wa.next_weight() == 1.0
    skipping = pkg.WeightAverage(model, start=2)
    assert skipping.next_weight() is None


def _randomise(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.randn(p.shape, generator=g))


def test_state_dict_round_trip():
    model = pkg.SimpleWakewordModel()
    wa = pkg.WeightAverage(model, mode="swa", decay=0.5, warmup=True, every="epoch", start=3)
    _randomise(wa.model, 1)
    wa.n_averaged, wa.n_calls = 4, 7
    sd = wa.state_dict()
    assert set(sd) >= {"mode", "decay", "warmup", "every", "start", "n_averaged", "parameters"}
    assert list(sd["parameters"]) == list(model.state_dict())
    other = pkg.WeightAverage(pkg.SimpleWakewordModel())
    other.load_state_dict(sd)
    assert (other.mode, other.decay, other.warmup, other.every, other.start, other.n_averaged, other.n_calls) == ("swa", 0.5, True, "epoch", 3, 4, 7)
    assert all(torch.equal(a, b) for a, b in zip(other.model.parameters(), wa.model.parameters())) and not other.model.training


def test_averaged_model_layout_round_trip():
    model = pkg.SimpleWakewordModel()
    wa = pkg.WeightAverage(model)
    _randomise(wa.model, 2)
    wa.n_averaged = 5
    sd = wa.to_averaged_model_state_dict()
    am = AveragedModel(pkg.SimpleWakewordModel())
    assert list(sd) == list(am.state_dict())                       # n_averaged, module.<key> ...: the layout, key for key
    am.load_state_dict(sd)
    assert int(am.n_averaged) == 5
    assert all(torch.equal(a, b) for a, b in zip(am.module.parameters(), wa.model.parameters()))
    am.n_averaged += 2
    _randomise(am.module, 3)
    back = pkg.WeightAverage(pkg.SimpleWakewordModel(), start=4)
    back.load_averaged_model_state_dict(am.state_dict())
    assert back.n_averaged == 7 and back.n_calls == 11
    assert all(torch.equal(a, b) for a, b in zip(back.model.parameters(), am.module.parameters()))
    assert not any(torch.equal(a, b) for a, b in zip(back.model.parameters(), wa.model.parameters()))
