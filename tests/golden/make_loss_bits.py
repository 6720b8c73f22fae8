"""Record the bits of the three cross-entropy entry points (ww_ce_loss_f32, ww_ce_loss_ex_f32, ww_ce_loss_soft_f32; csrc/ww_optim.hip):

    PYTHONPATH=. python tests/golden/make_loss_bits.py [--commit SHA] [--out tests/golden/loss_bits.json]

Run it on the MI355X on a build of a commit whose loss code is TRUSTED -- the commit before a change to the loss kernels, never the
code under test: tests/test_gpu_loss_bits.py compares the build it tests with this record, bit for bit.  The file names the commit
(`git rev-parse HEAD`, or --commit where the tree travels without its history) and the sha256 of csrc/ww_optim.hip as built, so that a
reader can check the record's origin against `git show <commit>:wakeword-jupyterlab_amd/csrc/ww_optim.hip`.

Per case the record holds the sha256 of the input bytes (a changed generator shows up as exactly that), the sha256 of dlogits, the loss
as its 32-bit pattern and the six words of the ww_loss_stats record (the first a float64 pattern).  The hashes depend on the ROCm device
math library (exp, log and the float64 division) as well as on this project's code.

Inputs: trainer_ref.ce_inputs(n, seed=n) and mixup_ref.soft_inputs(n, seed=n) with, at fixed clips, a few bad labels or rows and one
non-finite logit.  The non-finite logit sits on clip 1, whose label (7) or row (NaN, NaN) is bad in every case: the clip is counted in
`nonfinite` and adds nothing, so the loss stays a finite number whose bits record the order of summation.

Every case runs twice: on tensors on the 16-byte grid, and with logits and dlogits 4 bytes off it, labels 8 bytes off it and
probabilities 4 bytes off it.  The two runs must agree in every bit, and the words around dlogits must stay as they were."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import loss_ref  # noqa: E402
import mixup_ref  # noqa: E402
import trainer_ref  # noqa: E402

OUT = os.path.join(HERE, "loss_bits.json")
SOURCE = os.path.join(ROOT, "wakeword-jupyterlab_amd", "csrc", "ww_optim.hip")
SIZES = loss_ref.SIZES + (511, 513)        # 511: 256 pairs, one per lane, an odd tail; 513: 257 pairs, lane 0 takes a second
GUARD = -77.25
W = dict(weight=(0.25, 4.0), label_smoothing=0.125)
# (tag, kernel, what replaces the targets, keywords of ops.ce_loss_into / ops.soft_ce_loss_into)
CASES = (
    ("plain", "labels", None, {}),
    ("ex weighted smoothed mean", "labels", None, dict(W)),
    ("ex weighted smoothed sum", "labels", None, dict(W, reduction="sum")),
    ("ex focal weighted", "labels", None, dict(focal_gamma=2.0, weight=(0.25, 4.0))),
    ("ex ignore_index=0", "labels", None, dict(ignore_index=0)),
    ("ex every label ignored", "labels", "none", dict(W)),
    ("soft", "probs", None, {}),
    ("soft weighted smoothed mean", "probs", None, dict(W)),
    ("soft weighted smoothed sum", "probs", None, dict(W, reduction="sum")),
    ("soft every row bad", "probs", "none", {}),
)


def inputs(n, kind, replace):
    """(logits [n, 2] float32, labels [n] int64 or probabilities [n, 2] float32) with the planted clips."""
    if kind == "labels":
        z, t = trainer_ref.ce_inputs(n, seed=n)
        t = t.copy()
        for i, bad in ((1, 7), (7, -100), (300, -3)):        # -100: a bad label to the plain call, an ignored one under any option
            if i < n:
                t[i] = bad
        if replace == "none":
            t[:] = -100
    else:
        z, t = mixup_ref.soft_inputs(n, seed=n)
        for i, bad in ((1, (np.nan, np.nan)), (7, (-0.25, 0.5)), (300, (np.inf, 0.0))):
            if i < n:
                t[i] = bad
        if replace == "none":
            t[:] = np.nan
    z = z.copy()
    if n > 1:
        z[1, 1] = np.inf
    return np.ascontiguousarray(z), np.ascontiguousarray(t)


def _off_grid(t, skip, dev):
    """A copy of `t` that starts `skip` elements after a 16-byte boundary (torch allocates on one)."""
    import torch
    buf = torch.zeros(t.numel() + skip, dtype=t.dtype, device=dev)
    buf[skip:] = t.reshape(-1)
    assert buf.data_ptr() % 16 == 0
    return buf[skip:].view(t.shape)


def _run(kind, z, t, d, opts, dev):
    import torch
    from wakeword_jupyterlab_amd import ops
    loss, stats = torch.zeros((), device=dev), ops.new_loss_stats(dev)
    (ops.ce_loss_into if kind == "labels" else ops.soft_ce_loss_into)(z, t, d, loss, stats, **opts)
    return {"dlogits": hashlib.sha256(d.cpu().numpy().tobytes()).hexdigest(), "loss": loss.cpu().numpy().view(np.uint32).item().to_bytes(4, "big").hex(),
            "stats": stats.cpu().tolist()}


def measure(n, tag, kind, replace, opts, dev):
    """One case's record from the loaded build.  AssertionError where the aligned and the off-grid run differ or a guard word moved."""
    import torch
    z, t = inputs(n, kind, replace)
    zt, tt = torch.from_numpy(z).to(dev), torch.from_numpy(t).to(dev)
    assert zt.data_ptr() % 16 == 0 and tt.data_ptr() % 16 == 0
    lead = {"aligned": 4, "off grid": 1}                    # floats in front of dlogits: on the 16-byte grid, 4 bytes off it
    runs = {}
    for name, (zz, yy) in (("aligned", (zt, tt)), ("off grid", (_off_grid(zt, 1, dev), _off_grid(tt, 1, dev)))):
        buf = torch.full((2 * n + 2 * lead[name],), GUARD, device=dev)
        d = buf[lead[name]:lead[name] + 2 * n].view(n, 2)
        assert d.data_ptr() % 16 == (0 if name == "aligned" else 4) and yy.data_ptr() % 16 == (0 if name == "aligned" else tt.element_size())
        runs[name] = _run(kind, zz, yy, d, opts, dev)
        assert torch.all(buf[:lead[name]] == GUARD) and torch.all(buf[lead[name] + 2 * n:] == GUARD), f"n={n} {tag}: {name}: a guard word of dlogits moved"
    assert runs["aligned"] == runs["off grid"], f"n={n} {tag}: aligned {runs['aligned']} != off grid {runs['off grid']}"
    return dict(runs["aligned"], inputs=hashlib.sha256(z.tobytes() + t.tobytes()).hexdigest())


def keys():
    return [(n,) + case for n in SIZES for case in CASES]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit of the build, where `git rev-parse HEAD` cannot tell")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
    dev = torch.device("cuda", 0)
    with open(SOURCE, "rb") as f:
        source = hashlib.sha256(f.read()).hexdigest()
    cases = {f"n={n} {tag}": measure(n, tag, kind, replace, opts, dev) for n, tag, kind, replace, opts in keys()}
    with open(a.out, "w") as f:
        f.write('{"commit": "%s",\n"ww_optim.hip": "%s",\n"cases": {\n' % (commit, source))
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in cases.items()))
        f.write("\n}}\n")
    print(f"{len(cases)} cases -> {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
