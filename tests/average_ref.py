"""What the averaged-weights tests share: the float64 recursion, the float32 reference and the error figure.

The rule is the project's (tests/trainer_ref.py): the reference for a float32 average is torch.lerp in float32 on the same device, fed the
SAME float32 parameter snapshots the kernel saw; both are compared with the float64 recursion over those snapshots; the reference's own
error stays under a fixed cap, ours under twice the reference's + 2^-24.  The error figure is the largest absolute difference divided by
the tensor set's largest |p|."""
import numpy as np

import trainer_ref as ref

U = ref.U

# Caps on the REFERENCE's error (float32 torch.lerp against the float64 recursion), by the number of updates: twice the largest figure
# measured on the MI355X over the cases of tests/test_gpu_average.py, rounded up to a whole u (u = 2^-24).  Measured there (torch 2.10,
# ROCm 7.0):  2 updates (epoch SWA) 0.75 u;  3 updates (weights 1, 0.1, 0.5 over the 16-tensor table) 0.86 u;  5 trainer steps at decay
# 0.99: 2.74 u (SimpleWakewordModel), 1.97 u (WakewordModel);  50 updates: 5.69 u (EMA 0.999), 2.50 u (EMA 0.9 with warmup), 6.65 u (SWA).
# For orientation, float32 torch.lerp on a CPU gave 1.4 u after 3 updates and 7.2 u after 50 at decay 0.999.
CAP_SHORT = 6 * U                                              # up to 5 updates
CAP_50 = 14 * U                                                # 50 updates


def recursion(snaps, weights):
    """The averaging rule in float64 over a list of parameter snapshots (arrays of one shape) and one weight per snapshot:
    w == 1 copies, w == 0 keeps, else torch.lerp's two branches."""
    a = None
    for p, w in zip(snaps, weights):
        p = np.asarray(p, np.float64)
        if w == 1.0:
            a = p.copy()
        elif w == 0.0:
            pass
        elif w < 0.5:
            a = a + w * (p - a)
        else:
            a = p - (1.0 - w) * (p - a)
    return a


def lerp_reference(snaps, weights):
    """The float32 reference on the snapshots' own device: torch.lerp(a, p, w) per update (w == 1: a copy).  `snaps`: torch tensors."""
    import torch
    a = None
    for p, w in zip(snaps, weights):
        if w == 1.0:
            a = p.clone()
        elif w != 0.0:
            a = torch.lerp(a, p, float(w))
    return a


def error(a, a64, pmax):
    return float(np.max(np.abs(np.asarray(a, np.float64) - a64))) / pmax


def rule(name, ours, reference, cap):
    print(f"{name}: ours {ours / U:.3f} u, torch.lerp {reference / U:.3f} u (u = 2^-24)")
    assert reference <= cap, f"{name}: the reference's own error {reference / U:.3f} u exceeds its cap {cap / U:.1f} u"
    assert ours <= ref.allowed(reference), f"{name}: {ours / U:.3f} u > 2 x {reference / U:.3f} u + 1 u"
