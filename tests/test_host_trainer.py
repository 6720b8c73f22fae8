"""WakewordTrainer / FusedAdam without a GPU: the new C entry points are bound with the header's prototypes
and refuse bad arguments before any HIP call, naming the field; the lazy exports resolve; TrainingConfig holds the reference's values;
the float64 restatements of tests/trainer_ref.py agree with torch on the CPU within the caps the GPU tests hold torch to."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import trainer_ref as ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ww_ce_loss_f32", "ww_adam_step_f32", "ww_grad_norm_workspace_bytes", "ww_grad_norm_f32")
L = nat.lib


def _err():
    return (L.ww_last_error() or b"").decode()


def test_abi_stays_4_and_new_symbols_are_bound():
    assert L.ww_abi_version() == 4 == nat.ABI_VERSION
    lib = C.CDLL(nat.LIB_PATH)
    for name in NEW:
        assert name in nat.PROTOTYPES and hasattr(lib, name)
        assert getattr(L, name).argtypes == nat.PROTOTYPES[name][1] and getattr(L, name).restype == nat.PROTOTYPES[name][0]
    assert nat.PROTOTYPES["ww_adam_step_f32"][1] == [C.POINTER(nat.AdamTensor), C.c_int64] + [C.c_double] * 5 + [C.c_int64, C.c_void_p, C.c_void_p]
    assert nat.PROTOTYPES["ww_ce_loss_f32"][1] == [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4


def test_structs_are_the_headers():
    text = open(os.path.join(ROOT, "include", "wakeword_amd.h")).read()
    ctype = {"double": C.c_double, "int64_t": C.c_int64, "float*": C.c_void_p, "const float*": C.c_void_p}
    for cname, cls, size in (("ww_loss_stats", nat.LossStats, 48), ("ww_adam_tensor", nat.AdamTensor, 40)):
        body = re.search(rf"typedef struct {cname} \{{(.*?)\}} {cname};", text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = re.findall(r"(const float\*|float\*|double|int64_t)\s+(\w+)\s*;", body)
        assert [(n, ctype[t]) for t, n in fields] == list(cls._fields_)
        assert C.sizeof(cls) == size and all(getattr(cls, n).offset == 8 * i for i, (_, n) in enumerate(fields))
    assert re.search(r"#define WW_ADAM_MAX_TENSORS 16\b", text) and nat.ADAM_MAX_TENSORS == 16
    from wakeword_jupyterlab_amd import ops
    assert ops.LOSS_STATS_FIELDS == tuple(n for n, _ in nat.LossStats._fields_)


def _table(**kw):
    tab = (nat.AdamTensor * 17)()
    for k in range(17):                                        # distinct, 4-byte aligned, never dereferenced: the checks come first
        tab[k].p, tab[k].g, tab[k].m, tab[k].v, tab[k].n = 0x10000 + k * 0x100, 0x20000 + k * 0x100, 0x30000 + k * 0x100, 0x40000 + k * 0x100, 8
    for k, v in kw.items():
        setattr(tab[0], k, v)
    return tab


def _adam(tab=None, n_tensors=2, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, step=1):
    return L.ww_adam_step_f32(_table() if tab is None else tab, n_tensors, lr, beta1, beta2, eps, wd, step, None, None)


@pytest.mark.parametrize("kw, word", [
    (dict(n_tensors=0), "n_tensors"), (dict(n_tensors=17), "n_tensors"), (dict(lr=float("nan")), "lr"), (dict(lr=-1e-3), "lr"),
    (dict(lr=float("inf")), "lr"), (dict(beta1=1.0), "beta1"), (dict(beta1=-0.1), "beta1"), (dict(beta2=1.0), "beta2"),
    (dict(beta2=float("nan")), "beta2"), (dict(eps=0.0), "eps"), (dict(eps=-1e-8), "eps"), (dict(wd=-1e-5), "weight_decay"),
    (dict(step=0), "step"), (dict(tab=_table(n=0)), "tensors[0].n"), (dict(tab=_table(n=-3)), "tensors[0].n"),
    (dict(tab=_table(p=None)), "null"), (dict(tab=_table(g=None)), "null"), (dict(tab=_table(m=None)), "null"), (dict(tab=_table(v=None)), "null"),
    (dict(tab=_table(p=0x10002)), "aligned"), (dict(tab=_table(m=0x10100)), "overlap"), (dict(tab=_table(v=0x3001c)), "overlap"),
])
def test_adam_refuses_before_any_hip_call(kw, word):
    assert _adam(**kw) == nat.WW_EINVAL and word in _err()


def test_adam_null_table_and_the_device_check_comes_last():
    assert L.ww_adam_step_f32(None, 2, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None) == nat.WW_EINVAL and "null" in _err()
    tab = _table()
    tab[1].g = tab[0].g                                        # two entries may share a gradient
    if not torch.cuda.is_available():
        assert _adam(tab=tab, n_tensors=16) == nat.WW_ENODEVICE


def test_ce_loss_refuses_before_any_hip_call():
    for n in (0, -1, 2 ** 30 + 1):
        assert L.ww_ce_loss_f32(16, 16, n, None, None, None, None) == nat.WW_EINVAL and "n " in _err()
    assert L.ww_ce_loss_f32(None, 16, 4, None, None, None, None) == nat.WW_EINVAL and "null" in _err()
    assert L.ww_ce_loss_f32(16, None, 4, None, None, None, None) == nat.WW_EINVAL and "null" in _err()
    assert L.ww_ce_loss_f32(18, 16, 4, None, None, None, None) == nat.WW_EINVAL and "aligned" in _err()
    assert L.ww_ce_loss_f32(16, 20, 4, None, None, None, None) == nat.WW_EINVAL and "aligned" in _err()
    assert L.ww_ce_loss_f32(16, 16, 4, None, None, 20, None) == nat.WW_EINVAL and "stats_dev" in _err()
    if not torch.cuda.is_available():
        assert L.ww_ce_loss_f32(16, 16, 4, None, None, None, None) == nat.WW_ENODEVICE


def test_grad_norm_refuses_before_any_hip_call():
    tab = _table()
    assert L.ww_grad_norm_workspace_bytes(tab, 0) == nat.WW_EINVAL and "n_tensors" in _err()
    assert L.ww_grad_norm_workspace_bytes(tab, 17) == nat.WW_EINVAL and "n_tensors" in _err()
    assert L.ww_grad_norm_workspace_bytes(None, 1) == nat.WW_EINVAL and "null" in _err()
    assert L.ww_grad_norm_workspace_bytes(tab, 16) == 256
    tab[0].n = 4096 * 40 - 3                                   # 40 partial sums of 8 bytes, + 15 one-block tensors
    assert L.ww_grad_norm_workspace_bytes(tab, 16) == 512
    for bad in (0.0, -1.0, float("nan")):
        assert L.ww_grad_norm_f32(tab, 2, bad, 16, 16, 256, None) == nat.WW_EINVAL and "max_norm" in _err()
    assert L.ww_grad_norm_f32(tab, 0, 1.0, 16, 16, 256, None) == nat.WW_EINVAL and "n_tensors" in _err()
    assert L.ww_grad_norm_f32(_table(n=0), 2, 1.0, 16, 16, 256, None) == nat.WW_EINVAL and "tensors[0].n" in _err()
    assert L.ww_grad_norm_f32(_table(g=None), 2, 1.0, 16, 16, 256, None) == nat.WW_EINVAL and "null" in _err()
    for args in ((None, 16, 256), (16, None, 256), (16, 16, None)):
        assert L.ww_grad_norm_f32(tab, 2, 1.0, *args, None) == nat.WW_EINVAL and "null" in _err()
    assert L.ww_grad_norm_f32(tab, 2, 1.0, 16, 16, 128, None) == nat.WW_EINVAL and "aligned" in _err()
    if not torch.cuda.is_available():                          # only g and n are read: a table without p, m and v passes the checks
        assert L.ww_grad_norm_f32(_table(p=None, m=None, v=None), 2, 1.0, 16, 16, 256, None) == nat.WW_ENODEVICE


@pytest.mark.parametrize("n_conv", [2, 3])
def test_train_grads_struct_points_at_the_named_gradients(n_conv):
    """ops.train_grads_struct, the one builder behind _TrainStep.backward and WakewordTrainer._bind_grads: every pointer field of
    ww_train_grads is the address of the gradient of that name (data_ptr() needs no device).  The struct's per-layer bias gradient is
    bias_ih's -- bias_hh shares it -- and weight_hh has no field: neither key is read, so neither tensor's address appears."""
    from wakeword_jupyterlab_amd import ops
    keys = ops._train_keys(n_conv)
    grads = {k: torch.zeros(3 + i) for i, k in enumerate(keys)}                 # distinct storages, distinct addresses
    assert len({g.data_ptr() for g in grads.values()}) == len(keys) == 10 + 2 * n_conv
    tg = ops.train_grads_struct(grads, n_conv)
    assert isinstance(tg, nat.TrainGrads)
    want = {"conv_weight": [grads[f"conv{i + 1}.weight"].data_ptr() if i < n_conv else None for i in range(3)],
            "conv_bias": [grads[f"conv{i + 1}.bias"].data_ptr() if i < n_conv else None for i in range(3)],
            "lstm_weight_ih": [grads[f"lstm.weight_ih_l{layer}"].data_ptr() for layer in range(2)],
            "lstm_bias": [grads[f"lstm.bias_ih_l{layer}"].data_ptr() for layer in range(2)],
            "fc_weight": grads["fc.weight"].data_ptr(), "fc_bias": grads["fc.bias"].data_ptr()}
    assert [name for name, _ in nat.TrainGrads._fields_] == list(want)
    got = {name: list(getattr(tg, name)) if isinstance(want[name], list) else getattr(tg, name) for name in want}
    assert got == want
    unread = [k for k in keys if "weight_hh" in k or "bias_hh" in k]
    assert len(unread) == 4
    held = {p for v in got.values() for p in (v if isinstance(v, list) else [v])}
    assert not held & {grads[k].data_ptr() for k in unread}
    ops.train_grads_struct({k: g for k, g in grads.items() if k not in unread}, n_conv)        # ... and the builder does not ask for them


def test_lazy_exports_and_training_config():
    from wakeword_jupyterlab_amd import config, optim, trainer
    assert pkg.WakewordTrainer is trainer.WakewordTrainer and pkg.FusedAdam is optim.FusedAdam and pkg.TrainingConfig is config.TrainingConfig
    assert pkg.optim is optim and pkg.trainer is trainer
    c = pkg.TrainingConfig
    assert (c.BATCH_SIZE, c.LEARNING_RATE, c.EPOCHS, c.VALIDATION_SPLIT, c.TEST_SPLIT) == (16, 0.0001, 10, 0.2, 0.1)
    assert issubclass(pkg.FusedAdam, torch.optim.Adam)


def test_fused_adam_constructor_refusals():
    w = [torch.nn.Parameter(torch.zeros(3))]
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True), dict(decoupled_weight_decay=True),
               dict(lr=torch.tensor(1e-3))):
        with pytest.raises(NotImplementedError):
            pkg.FusedAdam(w, **kw)
    with pytest.raises(ValueError):
        pkg.FusedAdam(w, eps=0.0)
    opt = pkg.FusedAdam(w, lr=1e-4, weight_decay=1e-5)
    assert opt.defaults["lr"] == 1e-4 and opt.defaults["weight_decay"] == 1e-5 and opt.defaults["betas"] == (0.9, 0.999)
    opt.step()                                                 # no gradient yet: nothing to launch
    w[0].grad = torch.zeros(3)
    with pytest.raises(RuntimeError, match="on the GPU"):      # a CPU parameter is refused on the first step that meets it
        opt.step()
    torch.optim.Adam(w).load_state_dict(pkg.FusedAdam(w).state_dict())


def test_trainer_refuses_other_models():
    with pytest.raises(TypeError):
        pkg.WakewordTrainer(torch.nn.Linear(4, 2), torch.device("cpu"))
    with pytest.raises(TypeError, match="CPU"):
        pkg.WakewordTrainer(pkg.SimpleWakewordModel(), torch.device("cpu"))


# ---- the float64 restatements against torch on the CPU, within the caps the GPU tests hold torch to -------------------------------
@pytest.mark.parametrize("lr", [1e-4, 1e-3])
@pytest.mark.parametrize("wd", [0.0, 1e-5])
def test_adam_restatement_agrees_with_torch(lr, wd):
    p0, gs = ref.adam_inputs(70001, seed=5)
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([p], lr=lr, weight_decay=wd, foreach=False)
    p64, m64, v64 = p0.astype(np.float64), np.zeros_like(p0, np.float64), np.zeros_like(p0, np.float64)
    gmax = 0.0
    for t in range(3):
        p.grad = torch.from_numpy(gs[t].copy())
        opt.step()
        p64, m64, v64, g1 = ref.adam_step(p64, gs[t], m64, v64, lr, 0.9, 0.999, 1e-8, wd, t + 1)
        gmax = max(gmax, float(np.abs(g1).max()))
        st = opt.state[p]
        ep, em, ev = ref.adam_errors(p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), p64, m64, v64, lr, gmax)
        assert ep <= ref.CAP_P and em <= ref.CAP_M and ev <= ref.CAP_V, (t, ep / ref.U, em / ref.U, ev / ref.U)


@pytest.mark.parametrize("labels", ["mixed", "zeros", "ones"])
def test_cross_entropy_restatement_agrees_with_torch(labels):
    z, y = ref.ce_inputs(4099, seed=3, labels=labels)
    zt = torch.from_numpy(z).requires_grad_()
    loss = F.cross_entropy(zt, torch.from_numpy(y))
    loss.backward()
    loss64, d64, correct = ref.ce(z, y)
    assert abs(float(loss.detach()) - loss64) <= ref.CAP_LOSS * abs(loss64)
    assert float(np.abs(zt.grad.numpy().astype(np.float64) - d64).max()) * len(y) <= ref.CAP_DLOGITS
    assert correct == int((torch.max(zt.detach(), 1)[1] == torch.from_numpy(y)).sum())
    # labels outside {0, 1} add nothing: the loss of the rest over the same n, exact zeros in the gradient
    y2 = y.copy()
    y2[::3] = 2
    y2[1::3] = -1
    loss2, d2, c2 = ref.ce(z, y2)
    keep = (y2 == 0) | (y2 == 1)
    assert np.all(d2[~keep] == 0.0) and np.array_equal(d2[keep], d64[keep])
    assert loss2 == pytest.approx(ref.ce(z[keep], y[keep])[0] * keep.sum() / len(y), rel=1e-12)


def test_clip_restatement_agrees_with_torch():
    rng = np.random.default_rng(0)
    gs = [rng.standard_normal(s).astype(np.float32) for s in (5, 1000, 33)]
    ps = [torch.nn.Parameter(torch.zeros(g.shape)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = torch.from_numpy(g.copy())
    norm = float(torch.nn.utils.clip_grad_norm_(ps, 1.0))
    n64, s64 = ref.clip(gs, 1.0)
    assert norm == pytest.approx(n64, rel=1e-6) and s64 < 1.0
    assert np.allclose(ps[1].grad.numpy(), gs[1] * s64, rtol=1e-6, atol=0)
    assert ref.clip(gs, 1e9)[1] == 1.0
