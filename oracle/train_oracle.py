"""Float64 statements of the training step, stage by stage, and the checker that compares a set of kernel intermediates with them.

Every stage function takes the stage's OWN inputs (what the kernel read) and returns what the kernel should have written, in
`dtype` (float64 by default; float32 gives the plain restatement whose own rounding error sizes some allowances).  The backward is
linear in the upstream gradient once its inputs are fixed, so a stage checked on its own input needs no budget for what happened
upstream of it -- the comparison can be as tight as the arithmetic of that one kernel.

Allowances (none is taken from the code under test):
  * GEMM element: (d + 3 + S) * 2^-24 * sum_k |a_k b_k|, see gemm_allowance;
  * gate backward: counted roundings, see gates_bwd_allowance;
  * head forward and conv stages: 4 x the error of the float32 restatement of the same stage on the same inputs (the margin
    tests/test_gpu_train.py grants the reference module's own float32 sums), + 2^-22 * sum |terms| for the split-precision kernels.
"""
import time

import numpy as np
import torch
import torch.nn.functional as F

H = 256
U = 2.0 ** -24            # unit roundoff of float32
F64, F32 = torch.float64, torch.float32


def _t(x, dtype=F64):
    return (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).detach().cpu().to(dtype)


# ------------------------------------------------------------------------------------------------
# head forward
# ------------------------------------------------------------------------------------------------
def gates_fwd(x, w_ih, b_ih, b_hh, dtype=F64):
    """x [n,K] -> [4,n,256]: sigmoid i, tanh g, sigmoid o, tanh c (c = i * g: c0 = 0, so the forget gate never enters)."""
    g = _t(x, dtype) @ _t(w_ih, dtype).T + (_t(b_ih, dtype) + _t(b_hh, dtype))
    gi, gg, go = torch.sigmoid(g[:, :H]), torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
    return torch.stack([gi, gg, go, torch.tanh(gi * gg)])


def hd_fwd(gates, mask, dtype=F64):
    g = _t(gates, dtype)
    return g[2] * g[3] * _t(mask, dtype)


def fc_fwd(hd1, w, b, dtype=F64):
    return _t(hd1, dtype) @ _t(w, dtype).T + _t(b, dtype)


# ------------------------------------------------------------------------------------------------
# head backward
# ------------------------------------------------------------------------------------------------
def gemm_tn(a, b, dtype=F64):
    """The weight-gradient form: a [K,M], b [K,N] -> (a^T b [M,N], column sums of a [M])."""
    a, b = _t(a, dtype), _t(b, dtype)
    return a.T @ b, a.sum(dim=0)


def gemm_nn(a, b, dtype=F64):
    return _t(a, dtype) @ _t(b, dtype)


def gates_bwd(dhd, gates, mask, dtype=F64):
    """The formula above lstm_gates_bwd_kernel: dh = dhd mask; d g_o = dh tc go (1 - go); dc = dh go (1 - tc^2);
    d g_i = dc gg gi (1 - gi); d g_g = dc gi (1 - gg^2); d g_f = 0.  -> [n, 1024] in torch's row order i, f, g, o."""
    g = _t(gates, dtype)
    gi, gg, go, tc = g[0], g[1], g[2], g[3]
    dh = _t(dhd, dtype) * _t(mask, dtype)
    dc = dh * go * (1 - tc * tc)
    return torch.cat([dc * gg * gi * (1 - gi), torch.zeros_like(dh), dc * gi * (1 - gg * gg), dh * tc * go * (1 - go)], dim=1)


def gates_bwd_allowance(dhd, gates, mask):
    """Roundings of the float32 evaluation, first order in u = 2^-24 (x 1.01 for the higher orders).  Each product or (1 - s) of a
    sigmoid costs one relative u.  fl(1 - fl(t t)) = (1 - t^2 (1 + d1)) (1 + d2) is off by at most u t^2 + u (1 - t^2) = u in
    ABSOLUTE terms (relative to 1 - t^2 that is unbounded as |t| -> 1), so the factors q = 1 - tc^2 and 1 - gg^2 carry an absolute u.
      dh = dhd m                    1 u
      dc = (dh go) q                2 more products: |err dc| <= |dh go| (u + 3 u q)         =: Bdc
      d g_i = dc gg gi (1 - gi)     3 products + (1 - gi): |gg gi (1 - gi)| Bdc + 4 u |d g_i|
      d g_g = (dc gi) (1 - gg^2)    2 products:            |gi| (1 - gg^2) Bdc + |dc gi| (u + 2 u (1 - gg^2))
      d g_o = dh tc go (1 - go)     dh, 3 products, (1 - go): 5 u |d g_o|
    Forget rows get 0: they must be exactly zero."""
    g = _t(gates)
    gi, gg, go, tc = g[0], g[1], g[2], g[3]
    dh = (_t(dhd) * _t(mask)).abs()
    q, qg = 1 - tc * tc, 1 - gg * gg
    dc = dh * go * q
    bdc = dh * go * (U + 3 * U * q)
    a_i = (gg * gi * (1 - gi)).abs() * bdc + 4 * U * (dc * gg * gi * (1 - gi)).abs()
    a_g = gi * qg * bdc + dc * gi * (U + 2 * U * qg)
    a_o = 5 * U * (dh * tc * go * (1 - go)).abs()
    return 1.01 * torch.cat([a_i, torch.zeros_like(dh), a_g, a_o], dim=1)


def splitk_plan(M, N, K, may_split=True):
    """sgemm()'s launch arithmetic (csrc/ww_train.hip): S slices of K, k pairs per slice, and the longest accumulation chain
    d = ceil(pairs per slice / 4) MFMA steps of one wave (the four waves of a workgroup take every fourth pair)."""
    tiles = ((N + 31) // 32) * ((M + 31) // 32)
    S = 1
    if may_split and K >= 512:
        while S < 8 and tiles * S < 1024 and K // (2 * S) >= 128:
            S *= 2
    per = ((K + 1) // 2 + S - 1) // S
    return S, per, (per + 3) // 4


def gemm_allowance(abs_a, abs_b, M, N, K, may_split=True, tn=True):
    """A-priori float32 bound of one element of mfma_gemm_kernel (+ combine_splitk_kernel).  A sum whose every term passes through at
    most D float32 additions is off by at most D u sum |terms| to first order.  A term's path here: its wave's accumulator, d MFMA
    steps (each adds the two products of a k pair with one rounding, the products themselves are exact in the MFMA's wider
    intermediate) -> the fixed-order sum of the four waves' tiles, 3 additions -> the slices in order, at most S - 1 <= S.
    Hence (d + 3 + S) u sum_k |a_k b_k|; nothing is measured.  The single rounding per v_mfma_f32_32x32x2_f32 step is an ASSUMPTION
    about the unit (the ISA text does not spell out its internal rounding); if it rounds after each of the two products the chain is
    2 d, not d.  The bound is worst-case linear in d while real rounding errors add like sqrt(d), so the measured ratios
    (profiles/train_stage_errors.json) show how much of it the kernels use under either reading.  The row sums follow the same path with b = 1 (the 8 = 4 waves x 2 k
    parities are paired in a tree of depth 4 <= 3 + 1), so the same form holds with |a_k|.
    -> (allowance of the product, allowance of the row sums or None)."""
    S, _, d = splitk_plan(M, N, K, may_split)
    f = (d + 3 + S) * U
    a, b = _t(abs_a).abs(), _t(abs_b).abs()
    if tn:
        return f * (a.T @ b), f * a.sum(dim=0)
    return f * (a @ b), None


def gp_of(dpooled, width, dtype=F64):
    return _t(dpooled, dtype) / (80 * width) if dtype == F64 else _t(dpooled, dtype) * torch.tensor(1.0 / (80 * width), dtype=dtype)


# ------------------------------------------------------------------------------------------------
# conv stages (images [n, C, 80, T])
# ------------------------------------------------------------------------------------------------
def conv1_act(mel, w1, b1, sign1=None, dtype=F64):
    """relu(conv1), the ReLU taken as z * sign1 where the kernel's own sign image is given (see replay_f64) -> (activation, z)."""
    z = F.conv2d(_t(mel, dtype), _t(w1, dtype), _t(b1, dtype), padding=1)
    return (z * _t(sign1, dtype) if sign1 is not None else F.relu(z)), z


def conv_wgrad(dz, act, dtype=F64):
    """dz [n,Co,80,T], act [n,Ci,80,T] -> (dW [Co,Ci,3,3], db [Co]) of a 3x3 convolution with padding 1."""
    dz, act = _t(dz, dtype), _t(act, dtype)
    return torch.nn.grad.conv2d_weight(act, (dz.shape[1], act.shape[1], 3, 3), dz, padding=1), dz.sum(dim=(0, 2, 3))


def rank_one_dz(gp, mask, dtype=F64):
    """The gradient behind the mean pool: gp[b, co] wherever the last conv's ReLU passed."""
    return _t(gp, dtype)[:, :, None, None] * _t(mask, dtype)


def conv_dgrad(dz, w, sign, dtype=F64):
    """d loss / d pre-activation of the layer below: (transposed conv of dz with w) * sign."""
    return F.conv_transpose2d(_t(dz, dtype), _t(w, dtype), padding=1) * _t(sign, dtype)


# ------------------------------------------------------------------------------------------------
# whole step
# ------------------------------------------------------------------------------------------------
def _forward(P, a, mask0, mask1, sign1, n_conv, keep_a1=False):
    a1 = z1 = None
    for li in range(1, n_conv + 1):
        z = F.conv2d(a, P[f"conv{li}.weight"], P[f"conv{li}.bias"], padding=1)
        a = z * sign1 if (li == 1 and sign1 is not None) else F.relu(z)
        if li == 1 and keep_a1:
            a.retain_grad()
            a1, z1 = a, z
    h = a.mean(dim=(2, 3))
    for layer, mask in ((0, mask0), (1, mask1)):
        g = h @ P[f"lstm.weight_ih_l{layer}"].T + P[f"lstm.bias_ih_l{layer}"] + P[f"lstm.bias_hh_l{layer}"]
        c = torch.sigmoid(g[:, :H]) * torch.tanh(g[:, 2 * H:3 * H])
        h = torch.sigmoid(g[:, 3 * H:]) * torch.tanh(c)
        h = h * mask
    return h @ P["fc.weight"].T + P["fc.bias"], a1, z1


def replay_f64(sd, x, labels, mask0, mask1, sign1=None):
    """The train-mode forward + CE loss in float64 torch with given dropout factors -> (loss, logits, {name: grad}).
    sign1 (bool [B, 32, 80, T], optional): conv1's ReLU taken as `z * sign1` -- the derivative the kernels used, where it differs from
    [z > 0] only at pre-activations that are zero to float32 rounding (the forward value changes by |z| ~ 1e-7 of its terms there)."""
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sd.items()}
    logits, _, _ = _forward(P, torch.tensor(x, dtype=torch.float64), torch.tensor(mask0, dtype=torch.float64),
                            torch.tensor(mask1, dtype=torch.float64), None if sign1 is None else torch.tensor(sign1, dtype=torch.float64),
                            3 if "conv3.weight" in sd else 2)
    loss = F.cross_entropy(logits, torch.tensor(labels))
    loss.backward()
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in P.items()}
    return float(loss), logits.detach().numpy(), grads


def replay_f64_chunked(sd, x, labels, mask0, mask1, sign1=None, chunk=256, flip_budget=False):
    """replay_f64 in chunks of at most `chunk` clips (reduction="sum" / B, .grad accumulated across chunks): host memory stays
    bounded at the benchmark batches.  flip_budget: also the per-entry budget of conv1's gradient for ReLU flips at pre-activations
    within 1e-6 of the magnitudes summed into them (tests/test_gpu_train.py::_conv1_flip_budget, here with the step's own dropout
    factors) -> (loss, logits, grads, budget or None, seconds)."""
    t0 = time.perf_counter()
    assert chunk <= 256
    B, T, n_conv = len(x), x.shape[3], 3 if "conv3.weight" in sd else 2
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sd.items()}
    mag = torch.tensor(np.abs(x).max() * np.abs(sd["conv1.weight"]).reshape(32, -1).sum(axis=1) + np.abs(sd["conv1.bias"]), dtype=F64)
    loss, logits = 0.0, []
    bw, bb = np.zeros((32, 1, 3, 3)), np.zeros(32)
    for s in range(0, B, chunk):
        e = min(B, s + chunk)
        lg, a1, z1 = _forward(P, _t(x[s:e]), _t(mask0[s:e]), _t(mask1[s:e]), None if sign1 is None else _t(sign1[s:e]), n_conv, flip_budget)
        part = F.cross_entropy(lg, torch.as_tensor(labels[s:e]), reduction="sum") / B
        part.backward()
        loss += float(part.detach())
        logits.append(lg.detach().numpy())
        if flip_budget:
            amb = (z1.detach().abs() <= 1e-6 * mag[None, :, None, None]).double()
            da = a1.grad.abs() * amb
            xp = F.pad(_t(x[s:e]).abs(), (1, 1, 1, 1))
            for dy in range(3):
                for dx in range(3):
                    bw[:, 0, dy, dx] += (da * xp[:, :, dy:dy + 80, dx:dx + T]).sum(dim=(0, 2, 3)).numpy()
            bb += da.sum(dim=(0, 2, 3)).numpy()
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in P.items()}
    budget = {"conv1.weight": bw, "conv1.bias": bb} if flip_budget else None
    return loss, np.concatenate(logits), grads, budget, time.perf_counter() - t0


# ------------------------------------------------------------------------------------------------
# the checker
# ------------------------------------------------------------------------------------------------
def ratio(got, want, allow):
    """max over the elements of |got - want| / allow; an element whose allowance is 0 must be exact (else inf)."""
    err = (_t(got) - _t(want)).abs()
    allow = torch.broadcast_to(_t(allow), err.shape)
    if bool(((allow == 0) & (err > 0)).any()) or not bool(torch.isfinite(err).all()):
        return float("inf")
    pos = allow > 0
    return float((err[pos] / allow[pos]).max()) if bool(pos.any()) else 0.0


def ratio_f32(got, want64, want32, extra=0.0):
    """Allowance 4 x the float32 restatement's own largest error over the tensor (+ `extra`, elementwise or scalar)."""
    own = float((_t(want32) - _t(want64)).abs().max())
    return ratio(got, want64, 4 * own + _t(extra))


def check_head(k, P, dlogits, grads, width):
    """k: the kernel's intermediates (ops.train_stages + mask0, mask1, logits), P: parameters (torch names), dlogits [n,2], grads: the
    parameter gradients the step returned.  Every stage against float64 on the kernel's own input -> {stage: error / allowance}."""
    n, C = k["pooled"].shape
    r = {}
    w0, w1, fw = P["lstm.weight_ih_l0"], P["lstm.weight_ih_l1"], P["fc.weight"]
    # forward
    for name, x, w, layer in (("gates0", k["pooled"], w0, 0), ("gates1", k["hd0"], w1, 1)):
        args = (x, w, P[f"lstm.bias_ih_l{layer}"], P[f"lstm.bias_hh_l{layer}"])
        r[name] = ratio_f32(k[name], gates_fwd(*args), gates_fwd(*args, dtype=F32))
    for name, g, m in (("hd0", k["gates0"], k["mask0"]), ("hd1", k["gates1"], k["mask1"])):
        r[name] = ratio_f32(k[name], hd_fwd(g, m), hd_fwd(g, m, dtype=F32))
    r["logits"] = ratio_f32(k["logits"], fc_fwd(k["hd1"], fw, P["fc.bias"]), fc_fwd(k["hd1"], fw, P["fc.bias"], dtype=F32))
    # fc backward
    dW, db = gemm_tn(dlogits, k["hd1"])
    aW, ab = gemm_allowance(dlogits, k["hd1"], 2, H, n)
    r["fc.weight"], r["fc.bias"] = ratio(grads["fc.weight"], dW, aW), ratio(grads["fc.bias"], db, ab)
    r["dhd1"] = ratio(k["dhd1"], gemm_nn(dlogits, fw), gemm_allowance(dlogits, fw, n, H, 2, False, tn=False)[0])
    # layer 1
    r["dg1"] = ratio(k["dg1"], gates_bwd(k["dhd1"], k["gates1"], k["mask1"]), gates_bwd_allowance(k["dhd1"], k["gates1"], k["mask1"]))
    dW, db = gemm_tn(k["dg1"], k["hd0"])
    aW, ab = gemm_allowance(k["dg1"], k["hd0"], 4 * H, H, n)
    r["weight_ih_l1"], r["bias_l1"] = ratio(grads["lstm.weight_ih_l1"], dW, aW), ratio(grads["lstm.bias_ih_l1"], db, ab)
    r["dhd0"] = ratio(k["dhd0"], gemm_nn(k["dg1"], w1), gemm_allowance(k["dg1"], w1, n, H, 4 * H, tn=False)[0])
    # layer 0
    r["dg0"] = ratio(k["dg0"], gates_bwd(k["dhd0"], k["gates0"], k["mask0"]), gates_bwd_allowance(k["dhd0"], k["gates0"], k["mask0"]))
    dW, db = gemm_tn(k["dg0"], k["pooled"])
    aW, ab = gemm_allowance(k["dg0"], k["pooled"], 4 * H, C, n)
    r["weight_ih_l0"], r["bias_l0"] = ratio(grads["lstm.weight_ih_l0"], dW, aW), ratio(grads["lstm.bias_ih_l0"], db, ab)
    r["dpooled"] = ratio(k["dpooled"], gemm_nn(k["dg0"], w0), gemm_allowance(k["dg0"], w0, n, C, 4 * H, tn=False)[0])
    # gp = dpooled * fl(1 / (80 width)): the constant's rounding and the product's, 2 u |gp| (x 1.01)
    gp = gp_of(k["dpooled"], width)
    r["gp"] = ratio(k["gp"], gp, 1.01 * 2 * U * gp.abs())
    for name in ("lstm.bias_hh_l0", "lstm.bias_hh_l1"):                         # d / d bias_hh is d / d bias_ih
        r[name] = 0.0 if np.array_equal(np.asarray(grads[name]), np.asarray(grads[name.replace("_hh_", "_ih_")])) else float("inf")
    return r


def _conv_pass(k, P, mel, sl, dt, absolute=False):
    """One pass over the clips `sl` in `dt`: every conv stage's sum over those clips from the kernel's own inputs -> {name: tensor},
    plus "dz2" (3-conv model: what the kernel's dz2 should be).  absolute: every operand as its magnitude -- sum |terms| of each stage."""
    n_conv = 3 if "conv3.weight" in P else 2
    val = (lambda v: _t(v, dt).abs()) if absolute else (lambda v: _t(v, dt))
    sign1 = None if k.get("sign1") is None else k["sign1"][sl]
    a1, z1 = conv1_act(mel[sl], P["conv1.weight"], P["conv1.bias"], sign1, dt)
    s1 = _t(sign1, dt) if sign1 is not None else (z1 > 0).to(dt)
    a1 = a1.abs() if absolute else a1
    dz_last = rank_one_dz(val(k["gp"][sl]), k["mask"][sl], dt)
    out = {}
    if n_conv == 2:
        dz2 = dz_last
    else:
        out["conv3.weight"], out["conv3.bias"] = conv_wgrad(dz_last, val(k["mid2"][sl]), dt)
        out["dz2"] = conv_dgrad(dz_last, val(P["conv3.weight"]), _t(k["mid2"][sl]) > 0, dt)
        dz2 = val(k["dz2"][sl])                                       # the stages below start from the kernel's own dz2
    out["conv2.weight"], out["conv2.bias"] = conv_wgrad(dz2, a1, dt)
    out["conv1.weight"], out["conv1.bias"] = conv_wgrad(conv_dgrad(dz2, val(P["conv2.weight"]), s1, dt), val(mel[sl]), dt)
    return out


def _image_pass(k, P, mel, sl, mag):
    """The kernel's own ReLU images against float64 on the clips `sl`, the criteria of tests/test_gpu_train.py: conv1's sign image may
    differ from [z > 0] only where |z| <= 1e-6 of the magnitudes summed into z; the last layer's image is compared with [z > 0] of the
    float64 pre-activation on the kernel's own input (relu(conv1) under its sign image; the 3-conv model: its own mid2).
    -> (sign flips, sign flips at unambiguous positions, last-layer flips), and for a kernel that keeps no sign image the conv1
    flip budget (weight, bias): the whole contribution |da1| |mel| of every ambiguous position may enter or leave."""
    n_conv = 3 if "conv3.weight" in P else 2
    sign1 = None if k.get("sign1") is None else k["sign1"][sl]
    a1, z1 = conv1_act(mel[sl], P["conv1.weight"], P["conv1.bias"], sign1)
    amb = z1.abs() <= 1e-6 * mag[None, :, None, None]
    flips = bad = 0
    budget = (0.0, 0.0)
    if sign1 is not None:
        flipped = _t(sign1, torch.bool) != (z1 > 0)
        flips, bad = int(flipped.sum()), int((flipped & ~amb).sum())
    else:
        dz2 = _t(k["dz2"][sl]) if n_conv == 3 else rank_one_dz(k["gp"][sl], k["mask"][sl])
        budget = conv_wgrad(conv_dgrad(dz2, P["conv2.weight"], amb).abs(), _t(mel[sl]).abs())
    top = f"conv{n_conv}"
    z_last = F.conv2d(_t(k["mid2"][sl]) if n_conv == 3 else a1, _t(P[f"{top}.weight"]), _t(P[f"{top}.bias"]), padding=1)
    return flips, bad, int((_t(k["mask"][sl], torch.bool) != (z_last > 0)).sum()), budget


def check_conv(k, P, mel, grads, split, chunk=256):
    """The conv stages.  k: gp [n,C], mask [n,C,80,T] (the kernel's own last-layer ReLU image), sign1 (the kernel's own conv1 sign
    image, or None for a kernel that keeps none: [z > 0] of float64 conv1, with the flip budget), 3-conv model: mid2, dz2 [n,64,80,T]
    (the kernel's own); mel [n,1,80,T]; grads: the step's conv gradients.  Three passes per chunk of clips (the stages are sums over
    clips): float64, the float32 restatement, and -- split precision only -- sum |terms| (each operand of those kernels is carried as
    two f16 halves, 22 bits: + 2^-22 sum |terms|).  The images the oracle adopts from the kernel are validated first (_image_pass):
    "sign1" = flips / (1e-5 of the positions), inf for a flip at an unambiguous position; "mask" = flips / (1e-5 of the positions).
    -> {stage: error / allowance}."""
    n, n_conv = len(mel), 3 if "conv3.weight" in P else 2
    names = [f"conv{i}.{p}" for i in range(1, n_conv + 1) for p in ("weight", "bias")]
    mag = _t(np.abs(np.asarray(mel)).max() * np.abs(np.asarray(P["conv1.weight"])).reshape(32, -1).sum(axis=1) + np.abs(np.asarray(P["conv1.bias"])))
    acc = {tag: {s: 0.0 for s in names} for tag in ("f64", "f32", "abs")}
    flips = bad = mask_flips = 0
    flip_w = flip_b = dz2_ratio = 0.0
    for s in range(0, n, chunk):
        sl = slice(s, min(n, s + chunk))
        f, b, m, (bw, bb) = _image_pass(k, P, mel, sl, mag)
        flips, bad, mask_flips, flip_w, flip_b = flips + f, bad + b, mask_flips + m, flip_w + bw, flip_b + bb
        p64, p32 = _conv_pass(k, P, mel, sl, F64), _conv_pass(k, P, mel, sl, F32)
        pab = _conv_pass(k, P, mel, sl, F64, absolute=True) if split else None
        for name in names:
            acc["f64"][name], acc["f32"][name] = acc["f64"][name] + p64[name], acc["f32"][name] + p32[name]
            if split:
                acc["abs"][name] = acc["abs"][name] + pab[name]
        if n_conv == 3:                                               # dz2 is elementwise per clip: checked chunk by chunk
            dz2_ratio = max(dz2_ratio, ratio_f32(k["dz2"][sl], p64["dz2"], p32["dz2"], 2.0 ** -22 * pab["dz2"] if split else 0.0))
    r = {}
    if k.get("sign1") is not None:
        r["sign1"] = float("inf") if bad else flips / (1e-5 * k["sign1"].numel())
    r["mask"] = mask_flips / (1e-5 * k["mask"].numel())
    for name in names:
        extra = 2.0 ** -22 * acc["abs"][name] if split else 0.0
        if name.startswith("conv1."):                                 # zero where the kernel's own sign image was used
            extra = extra + 1.01 * (flip_w if name.endswith("weight") else flip_b)
        r[name] = ratio_f32(grads[name], acc["f64"][name], acc["f32"][name], extra)
    if n_conv == 3:
        r["dz2"] = dz2_ratio
    return r
