"""The training backward stage by stage, and at the benchmark batch sizes.

The workspace of a step keeps almost every intermediate (ops.train_stages), and the backward is linear in the upstream gradient once
its inputs are fixed: every kernel is compared with float64 ON ITS OWN INPUT (oracle/train_oracle.py), far more tightly than the
end-to-end tolerances of tests/test_gpu_train.py allow, and at the batches whose split-K slices, persistent-group walks and partial
reductions only ever ran under bench.py's timer (4096 clips of the 2-conv model, 2048 of the 3-conv one).

Allowances -- none comes from the code under test (derivations beside the formulas in oracle/train_oracle.py):
  GEMM element   (d + 3 + S) 2^-24 sum_k |a_k b_k|: d = ceil(k pairs per slice / 4) MFMA steps, 3 = the wave combine, S = the slices
  row sums       the same form with |a_k|
  gate backward  counted roundings: 2^-24 relative per factor, an absolute 2^-24 on 1 - tc^2 and 1 - g^2; forget rows exactly 0
  gp             2 x 2^-24 |gp| (the constant 1 / (80 width) and the product)
  head forward, conv stages   4 x the error of a float32 torch restatement of the same stage on the same inputs (the margin
                 test_gradients_match_the_reference_module grants the reference's own float32 sums); split precision: + 2^-22 sum |terms|;
                 exact fp32 (no sign image kept): conv1 gets the flip budget of test_split_precision_backward_agrees_with_exact_fp32
tests/test_host_train_stages.py shows on the CPU that a float32 stand-in passes all of them and that each of nine injected faults fails.

Every ratio error / allowance is printed; with WW_TRAIN_STAGE_JSON=path the module writes them to that file (profiles/train_stage_errors.json)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wakeword_jupyterlab_amd as pkg
from oracle import train_oracle as orc
from wakeword_jupyterlab_amd import ops

pytestmark = pytest.mark.gpu
FIGURES = []


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _keep_workspaces_and_write_figures():
    ops.keep_train_workspace(True)
    yield
    ops.keep_train_workspace(False)
    ops.set_train_math("f16x3")
    path = os.environ.get("WW_TRAIN_STAGE_JSON")
    if path and FIGURES:
        with open(path, "w") as f:
            json.dump(FIGURES, f, indent=1)


@pytest.fixture(params=["f16x3", "f32"])
def train_math(request):
    ops.set_train_math(request.param)
    yield request.param
    ops.set_train_math("f16x3")


def _step(dev, arch, batch, width, math, stage_names):
    """One training step with dropout on (0.5 / 0.6) and scaled head weights, as test_train_step_with_dropout_replayed_in_float64."""
    sd = pkg.synth.make_state_dict(arch, seed=5)
    for k in sd:
        if "lstm" in k or k.startswith("fc"):
            sd[k] = (sd[k] * 3).astype(np.float32)
    m = pkg.WakewordModel() if arch == "full" else pkg.SimpleWakewordModel()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(dev).train()
    assert m.lstm.dropout == m.dropout.p == (0.6 if arch == "full" else 0.5)
    x = (pkg.synth.normal(3, batch * 80 * width).astype(np.float32).reshape(batch, 1, 80, width) * 15 - 35)
    labels = (np.arange(batch) % 2).astype(np.int64)
    torch.manual_seed(11)
    out = m(torch.from_numpy(x).to(dev))
    out.retain_grad()
    F.cross_entropy(out, torch.from_numpy(labels).to(dev)).backward()
    st = ops.train_stages(math, names=stage_names)
    grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    m0, m1 = (t.cpu() for t in ops.train_last_masks(batch))
    return sd, x, labels, out.detach().cpu(), out.grad.detach().cpu(), st, grads, m0, m1


def _record(kind, arch, math, batch, width, r):
    print(f"{kind} {arch} {math} batch {batch} width {width}: " + "  ".join(f"{k} {v:.3f}" for k, v in r.items()))
    FIGURES.append({"kind": kind, "arch": arch, "train_math": math, "batch": batch, "width": width, "ratios": r})
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, f"{kind} stages beyond their allowance ({arch}, {math}, batch {batch}, width {width}): {bad}"


HEAD_STAGES = ("pooled", "gates0", "gates1", "hd0", "hd1", "dhd1", "dg1", "dhd0", "dg0", "dpooled", "gp")
BATCHES = (1, 2, 37, 300, 511, 512, 513, 1023, 1024, 2049, 4096)
HEAD_CASES = [(a, b, 32) for a in ("simple", "full") for b in BATCHES if not (a == "full" and b > 2049)] + \
             [(a, b, w) for a in ("simple", "full") for b in (37, 513) for w in (9, 31)]


@pytest.mark.parametrize("arch,batch,width", HEAD_CASES)
def test_head_stages_against_float64_on_their_own_input(dev, arch, batch, width, train_math):
    sd, _, _, logits, dlogits, st, grads, m0, m1 = _step(dev, arch, batch, width, train_math, HEAD_STAGES)
    k = {n: t.cpu() for n, t in st.items()}
    k.update(mask0=m0, mask1=m1, logits=logits)
    P = {n: torch.from_numpy(v) for n, v in sd.items()}
    _record("head", arch, train_math, batch, width, orc.check_head(k, P, dlogits, grads, width))


def _conv_inputs(st, math, arch, batch, width):
    """The kernel's own inputs of the conv stages, [n, C, 80, width]: gp, the last layer's ReLU image, conv1's sign image (split
    precision; the exact-fp32 kernels keep none), and for the 3-conv model mid2 and dz2."""
    k = {"gp": st["gp"].cpu()}
    if math == "f16x3":
        mask, sign1 = (t.cpu().numpy() for t in ops.train_last_bit_images())
        k["mask"] = torch.from_numpy(np.unpackbits(mask, axis=-1, bitorder="little")).permute(0, 3, 1, 2)[..., :width].bool()
        words = sign1.astype(np.uint32)
        k["sign1"] = torch.from_numpy(np.ascontiguousarray((((words[..., None] >> np.arange(32, dtype=np.uint32)) & 1) != 0)
                                                           .transpose(0, 3, 1, 2)[..., :width]))
    else:                                                # exact fp32 keeps the activation itself, and its backward takes [act > 0] from it
        k["mask"] = (st["mid3" if arch == "full" else "mid2"][..., :width] > 0).cpu()
        k["sign1"] = None
    if arch == "full":
        k["mid2"], k["dz2"] = st["mid2"][..., :width].cpu(), st["dz2"][..., :width].cpu()
    return k


def _conv_stage_names(arch, math):
    return ("gp",) + (("mid2", "dz2") if arch == "full" else ()) + ((("mid3",) if arch == "full" else ("mid2",)) if math == "f32" else ())


@pytest.mark.parametrize("arch", ["simple", "full"])
@pytest.mark.parametrize("batch", [3, 37, 300])
@pytest.mark.parametrize("width", [9, 17, 31, 32])
def test_conv_stages_against_float64_on_their_own_input(dev, arch, batch, width, train_math):
    sd, x, _, _, _, st, grads, _, _ = _step(dev, arch, batch, width, train_math, _conv_stage_names(arch, train_math))
    k = _conv_inputs(st, train_math, arch, batch, width)
    P = {n: torch.from_numpy(v) for n, v in sd.items()}
    _record("conv", arch, train_math, batch, width, orc.check_conv(k, P, torch.from_numpy(x), grads, split=train_math == "f16x3"))


@pytest.mark.parametrize("arch,batch", [("simple", 4096), ("full", 2048)])
def test_benchmark_batch_conv_stages_and_whole_step(dev, arch, batch):
    """bench.py's batches: the conv stages under both arithmetics, and the whole step's parameter gradients against the chunked float64
    replay (the kernel's masks in both modes, its sign image in split mode, the flip budget in fp32 mode) under the criteria of
    test_split_precision_backward_agrees_with_exact_fp32: the split-precision kernels no further from float64 than 2 x the exact-fp32
    kernels + 1e-5 of the tensor's largest gradient."""
    width, got, masks, sign1 = 32, {}, {}, None
    for math in ("f32", "f16x3"):
        ops.set_train_math(math)
        sd, x, labels, logits, dlogits, st, grads, m0, m1 = _step(dev, arch, batch, width, math, HEAD_STAGES + _conv_stage_names(arch, math))
        P = {n: torch.from_numpy(v) for n, v in sd.items()}
        kh = {n: st[n].cpu() for n in HEAD_STAGES}
        kh.update(mask0=m0, mask1=m1, logits=logits)
        _record("head", arch, math, batch, width, orc.check_head(kh, P, dlogits, grads, width))      # the head both arithmetics share
        k = _conv_inputs(st, math, arch, batch, width)
        del st, kh
        _record("conv", arch, math, batch, width, orc.check_conv(k, P, torch.from_numpy(x), grads, split=math == "f16x3"))
        got[math], masks[math] = {n: g.numpy().astype(np.float64) for n, g in grads.items()}, (m0.numpy(), m1.numpy())
        if math == "f16x3":
            sign1 = k["sign1"].numpy()
        del k
    assert all(np.array_equal(a, b) for a, b in zip(masks["f32"], masks["f16x3"]))         # the same seed: the same dropout factors
    m0, m1 = masks["f32"]
    _, _, exact, budget, t_a = orc.replay_f64_chunked(sd, x, labels, m0, m1, flip_budget=True)
    _, _, exact_h, _, t_b = orc.replay_f64_chunked(sd, x, labels, m0, m1, sign1=sign1)
    print(f"float64 replays of {batch} clips ({arch}): {t_a:.1f} s with the flip budget, {t_b:.1f} s with the sign image")
    fig = {"kind": "whole_step", "arch": arch, "batch": batch, "replay_seconds": [t_a, t_b], "errors": {}}
    FIGURES.append(fig)
    bad = []
    for name, g32 in got["f32"].items():
        ex, exh, gh = exact[name], exact_h[name], got["f16x3"][name]
        scale = np.abs(ex).max()
        if scale == 0.0:
            assert not gh.any() and not g32.any(), name
            continue
        assert np.isfinite(gh).all(), name
        e32 = np.abs(g32 - ex) / scale
        e32 = float(np.maximum(e32 - (1.01 * budget[name] / scale if name in budget else 0.0), 0.0).max())
        eh = float(np.abs(gh - exh).max() / scale)
        fig["errors"][name] = {"f32": e32, "f16x3": eh}
        print(f"  {name:22s} fp32 kernels {e32:.2e}   split {eh:.2e} of the largest gradient")
        # + an absolute ceiling, so that a fault both arithmetics share cannot hide in the relative criterion: _check_grads' 5e-4
        if not (eh <= 2 * e32 + 1e-5 and e32 <= 5e-4 and eh <= 5e-4):
            bad.append((name, e32, eh))
    assert not bad, bad


def test_stages_of_another_arithmetic_or_before_the_backward_are_refused(dev):
    """ww_train_stage reads the workspace by the layout of the arithmetic its forward ran under, and the d... stages only after the
    backward has written them: the other arithmetic and a read between forward and backward are errors, not stale bytes."""
    sd = pkg.synth.make_state_dict("simple", seed=3)
    m = pkg.SimpleWakewordModel()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(dev).train()
    x = torch.zeros(4, 1, 80, 32, device=dev) - 30.0
    for math, other in (("f16x3", "f32"), ("f32", "f16x3")):
        ops.set_train_math(math)
        out = m(x)
        assert set(ops.train_stages(math, names=("pooled", "hd1"))) == {"pooled", "hd1"}        # forward stages: readable at once
        with pytest.raises(RuntimeError, match="none has run"):
            ops.train_stages(math, names=("dg1",))
        F.cross_entropy(out, torch.tensor([0, 1, 0, 1], device=dev)).backward()
        assert ops.train_stages(math, names=("dg1",))["dg1"].shape == (4, 1024)
        with pytest.raises(RuntimeError, match="ran under train math"):
            ops.train_stages(other)
        with pytest.raises(ValueError):
            ops.train_stages("bf16")
    ops.set_train_math("f16x3")
