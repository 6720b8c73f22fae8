"""The stage checker of oracle/train_oracle.py, kept honest without a GPU: a float32 restatement of the training step stands in for the
kernels (split K, persistent groups and all).  It must pass every stage at the allowances the GPU test uses, and each fault below,
injected into it one at a time, must be rejected (tests/test_gpu_train_stages.py runs the same checker on the kernels' own numbers)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wakeword_jupyterlab_amd as pkg
from oracle import train_oracle as orc

F32 = torch.float32
H = 256


def _params(arch):
    sd = pkg.synth.make_state_dict(arch, seed=5)
    for k in sd:
        if "lstm" in k or k.startswith("fc"):
            sd[k] = (sd[k] * 3).astype(np.float32)
    return sd


def _masks(n, p, seed):
    rng = np.random.default_rng(seed)
    return ((rng.random((n, H)) >= p) / (1.0 - p)).astype(np.float32), ((rng.random((n, H)) >= p) / (1.0 - p)).astype(np.float32)


def _gemm32_tn(a, b, fault=None):
    """a [K,M], b [K,N] float32 -> (a^T b, column sums of a) the way sgemm() splits K: S slices of k pairs, summed in order."""
    K, M, N = a.shape[0], a.shape[1], b.shape[1]
    S, per, _ = orc.splitk_plan(M, N, K)
    k_end = K - 1 if (fault == "last_k" and K % 2) else K
    c, rs = torch.zeros(M, N), torch.zeros(M)
    for z in range(S):
        k0, k1 = 2 * z * per, min(2 * (z + 1) * per, k_end)
        if not (fault == "slice" and z == 1):
            c = c + a[k0:k1].T @ b[k0:k1]
        if not (fault == "rowsum_slice" and z == 1):
            rs = rs + a[k0:k1].sum(dim=0)
    return c, rs


def _standin_head(sd, n, width, fault=None):
    arch3 = "conv3.weight" in sd
    C = 128 if arch3 else 64
    P = {k: torch.from_numpy(v) for k, v in sd.items()}
    k = {"pooled": torch.from_numpy(np.abs(pkg.synth.normal(7, n * C).astype(np.float32).reshape(n, C)) * 0.3)}
    m0, m1 = _masks(n, 0.6 if arch3 else 0.5, 3)
    k["mask0"], k["mask1"] = torch.from_numpy(m0), torch.from_numpy(m1)
    for layer, x in ((0, "pooled"), (1, "hd0")):
        k[f"gates{layer}"] = orc.gates_fwd(k[x], P[f"lstm.weight_ih_l{layer}"], P[f"lstm.bias_ih_l{layer}"], P[f"lstm.bias_hh_l{layer}"], dtype=F32)
        k[f"hd{layer}"] = orc.hd_fwd(k[f"gates{layer}"], k[f"mask{layer}"], dtype=F32)
    k["logits"] = orc.fc_fwd(k["hd1"], P["fc.weight"], P["fc.bias"], dtype=F32)
    labels = torch.arange(n) % 2
    dlogits = (torch.softmax(k["logits"], dim=1) - F.one_hot(labels, 2).float()) / n
    g = {}
    g["fc.weight"], g["fc.bias"] = _gemm32_tn(dlogits, k["hd1"])
    k["dhd1"] = dlogits @ P["fc.weight"]
    k["dg1"] = orc.gates_bwd(k["dhd1"], k["gates1"], k["mask1"], dtype=F32)
    if fault == "forget":
        k["dg1"][n // 2, H + 5] = 1e-20
    g["lstm.weight_ih_l1"], g["lstm.bias_ih_l1"] = _gemm32_tn(k["dg1"], k["hd0"], fault)
    k["dhd0"] = k["dg1"] @ P["lstm.weight_ih_l1"]
    k["dg0"] = orc.gates_bwd(k["dhd0"], k["gates0"], k["mask0"], dtype=F32)
    g["lstm.weight_ih_l0"], g["lstm.bias_ih_l0"] = _gemm32_tn(k["dg0"], k["pooled"])
    k["dpooled"] = k["dg0"] @ P["lstm.weight_ih_l0"]
    k["gp"] = orc.gp_of(k["dpooled"], 32 if fault == "gp_width" else width, dtype=F32)
    g["lstm.bias_hh_l0"], g["lstm.bias_hh_l1"] = g["lstm.bias_ih_l0"].clone(), g["lstm.bias_ih_l1"].clone()
    return k, P, dlogits, g


def _standin_conv(sd, n, width, fault=None, groups=2):
    """float32 conv stages; the clips are dealt to `groups` persistent groups (clip g, g + groups, ...), each sums its own partial."""
    n_conv = 3 if "conv3.weight" in sd else 2
    C = 128 if n_conv == 3 else 64
    P = {k: torch.from_numpy(v) for k, v in sd.items()}
    mel = torch.from_numpy(pkg.synth.normal(3, n * 80 * width).astype(np.float32).reshape(n, 1, 80, width) * 15 - 35)
    a1, z1 = orc.conv1_act(mel, P["conv1.weight"], P["conv1.bias"], dtype=F32)
    a2 = F.relu(F.conv2d(a1, P["conv2.weight"], P["conv2.bias"], padding=1))
    last = F.relu(F.conv2d(a2, P["conv3.weight"], P["conv3.bias"], padding=1)) if n_conv == 3 else a2
    k = {"mask": last > 0, "sign1": z1 > 0}
    dpooled = torch.from_numpy(pkg.synth.normal(9, n * C).astype(np.float32).reshape(n, C) * 1e-4)
    k["gp"] = orc.gp_of(dpooled, width, dtype=F32)
    mask = torch.roll(k["mask"], 1, dims=1) if fault == "mask_shift" else k["mask"]
    dz_last = orc.rank_one_dz(k["gp"], mask, dtype=F32)
    if fault == "right_col":
        dz_last = dz_last.clone()
        dz_last[..., width - 1] = 0
    def grouped(dz, act, drop_last_of_group0=False):
        dw, db = 0.0, 0.0
        for gidx in range(groups):
            clips = list(range(gidx, n, groups))
            if drop_last_of_group0 and gidx == 0:
                clips = clips[:-1]
            if clips:
                w_, b_ = orc.conv_wgrad(dz[clips], act[clips], dtype=F32)
                dw, db = dw + w_, db + b_
        return dw, db
    g = {}
    top = f"conv{n_conv}"
    g[f"{top}.weight"], g[f"{top}.bias"] = grouped(dz_last, a2 if n_conv == 3 else a1, fault == "group_last_clip")
    if fault == "group_last_clip":
        g[f"{top}.bias"] = dz_last.sum(dim=(0, 2, 3))
    if fault == "bias_from_dpooled":
        g[f"{top}.bias"] = dpooled.sum(dim=0)
    dz2 = orc.rank_one_dz(k["gp"], k["mask"], dtype=F32)        # the faults sit in the weight-gradient kernel alone
    if n_conv == 3:
        k["mid2"] = a2
        k["dz2"] = dz2 = orc.conv_dgrad(orc.rank_one_dz(k["gp"], k["mask"], dtype=F32), P["conv3.weight"], a2 > 0, dtype=F32)
        g["conv2.weight"], g["conv2.bias"] = grouped(dz2, a1)
    g["conv1.weight"], g["conv1.bias"] = grouped(orc.conv_dgrad(dz2, P["conv2.weight"], k["sign1"], dtype=F32), mel)
    return k, P, mel, g


def _worst(r):
    return max(r.values()), max(r, key=r.get)


@pytest.mark.parametrize("arch", ["simple", "full"])
@pytest.mark.parametrize("n,width", [(37, 32), (513, 32), (37, 31), (513, 9)])
def test_float32_standin_passes_every_head_stage(arch, n, width):
    r = orc.check_head(*_standin_head(_params(arch), n, width), width)
    print({k: round(v, 3) for k, v in r.items()})
    assert _worst(r)[0] <= 1.0, _worst(r)


@pytest.mark.parametrize("arch", ["simple", "full"])
@pytest.mark.parametrize("width", [9, 17, 31, 32])
@pytest.mark.parametrize("own_sign", [True, False])
def test_float32_standin_passes_every_conv_stage(arch, width, own_sign):
    k, P, mel, g = _standin_conv(_params(arch), 3, width)
    if not own_sign:                                     # the exact-fp32 kernels keep no sign image: float64's own, with the flip budget
        k["sign1"] = None
    r = orc.check_conv(k, P, mel, g, split=False)
    print({k_: round(v, 3) for k_, v in r.items()})
    assert _worst(r)[0] <= 1.0, _worst(r)


HEAD_FAULTS = {"slice": ("one split-K slice dropped from a weight GEMM", 513, 32, ("weight_ih_l1",)),
               "rowsum_slice": ("one slice dropped from its row sum only", 513, 32, ("bias_l1",)),
               "last_k": ("the last k dropped when K is odd", 513, 32, ("weight_ih_l1", "bias_l1")),
               "forget": ("a forget-gate row that is not zero", 37, 32, ("dg1",)),
               "gp_width": ("gp scaled by 80*32 at width 31", 37, 31, ("gp",))}


@pytest.mark.parametrize("arch", ["simple", "full"])
@pytest.mark.parametrize("fault", sorted(HEAD_FAULTS))
def test_head_faults_are_rejected(arch, fault):
    what, n, width, stages = HEAD_FAULTS[fault]
    r = orc.check_head(*_standin_head(_params(arch), n, width, fault), width)
    for s in stages:
        assert r[s] > 1.0, f"{what}: stage {s} passed with ratio {r[s]:.3g}"
    for s, v in r.items():                               # and only the stage that holds the fault complains: the checks isolate it
        if s not in stages:
            assert v <= 1.0, (what, s, v)


CONV_FAULTS = {"group_last_clip": ("the last clip of one persistent group left out of a conv weight gradient", 32, ("weight",)),
               "right_col": ("the rightmost column dropped at width 31", 31, ("weight", "bias")),
               "mask_shift": ("one mask bit plane shifted by one channel", 32, ("weight", "bias")),
               "bias_from_dpooled": ("the last-layer bias gradient built from dpooled in place of the masked sum", 32, ("bias",))}


@pytest.mark.parametrize("arch", ["simple", "full"])
@pytest.mark.parametrize("fault", sorted(CONV_FAULTS))
def test_conv_faults_are_rejected(arch, fault):
    """Under the WIDER of the two allowances (split precision: + 2^-22 sum |terms|)."""
    what, width, parts = CONV_FAULTS[fault]
    k, P, mel, g = _standin_conv(_params(arch), 3, width, fault)
    r = orc.check_conv(k, P, mel, g, split=True)
    top = "conv3" if arch == "full" else "conv2"
    for p in parts:
        assert r[f"{top}.{p}"] > 1.0, f"{what}: {top}.{p} passed with ratio {r[f'{top}.{p}']:.3g}"
    for s, v in r.items():
        if s not in [f"{top}.{p}" for p in parts]:
            assert v <= 1.0, (what, s, v)


@pytest.mark.parametrize("arch", ["simple", "full"])
def test_chunked_replay_equals_the_whole_batch_replay(arch):
    """replay_f64_chunked (reduction="sum" / B, .grad accumulated) is the same float64 step as replay_f64, with or without a sign image."""
    sd, n, width = _params(arch), 5, 9
    x = (pkg.synth.normal(3, n * 80 * width).astype(np.float32).reshape(n, 1, 80, width) * 15 - 35)
    labels = (np.arange(n) % 2).astype(np.int64)
    m0, m1 = _masks(n, 0.5, 1)
    z1 = F.conv2d(torch.from_numpy(x), torch.from_numpy(sd["conv1.weight"]), torch.from_numpy(sd["conv1.bias"]), padding=1)
    for sign1 in (None, (z1 > 0).numpy()):
        loss, logits, grads = orc.replay_f64(sd, x, labels, m0, m1, sign1)
        loss_c, logits_c, grads_c, budget, _ = orc.replay_f64_chunked(sd, x, labels, m0, m1, sign1, chunk=2, flip_budget=sign1 is None)
        assert abs(loss - loss_c) <= 1e-13 and np.abs(logits - logits_c).max() <= 1e-13
        for name, g in grads.items():
            assert np.abs(g - grads_c[name]).max() <= 1e-12 * max(np.abs(g).max(), 1e-300), name
        assert budget is None or (budget["conv1.weight"].shape == (32, 1, 3, 3) and (budget["conv1.bias"] >= 0).all())
