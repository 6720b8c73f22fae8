"""Bit-equality of the training step between two checkouts (a change that must not alter any kernel, launch or workspace byte).

    python scripts/train_bitequal.py dump OUT.npz      in each tree: one seeded training step per model and arithmetic, at a batch
                                                      without split K (37 clips, width 31) and one with it (600 clips), dropout on;
                                                      logits and every parameter gradient
    python scripts/train_bitequal.py compare A.npz B.npz [A/logits.npy B/logits.npy]
                                                      every array bit for bit; the optional pair: bench.py --dump-outputs of both trees
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(path):
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F

    import wakeword_jupyterlab_amd as pkg
    from wakeword_jupyterlab_amd import ops

    assert os.path.abspath(pkg.__file__).startswith(ROOT), pkg.__file__
    dev = torch.device("cuda", 0)
    out = {}
    for arch in ("simple", "full"):
        for math in ("f32", "f16x3"):
            for batch, width in ((37, 31), (600, 32)):
                ops.set_train_math(math)
                sd = pkg.synth.make_state_dict(arch, seed=5)
                m = pkg.WakewordModel() if arch == "full" else pkg.SimpleWakewordModel()
                m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
                m = m.to(dev).train()
                x = (pkg.synth.normal(3, batch * 80 * width).astype(np.float32).reshape(batch, 1, 80, width) * 15 - 35)
                y = torch.from_numpy((np.arange(batch) % 2).astype(np.int64)).to(dev)
                torch.manual_seed(11)
                lg = m(torch.from_numpy(x).to(dev))
                F.cross_entropy(lg, y).backward()
                tag = f"{arch}.{math}.{batch}"
                out[f"{tag}.logits"] = lg.detach().cpu().numpy()
                for k, p in m.named_parameters():
                    out[f"{tag}.{k}"] = p.grad.cpu().numpy()
    torch.cuda.synchronize()
    np.savez(path, **out)
    print("dumped", len(out), "arrays from", ROOT)


def compare(a_path, b_path, logits=None):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files)
    bad = [k for k in a.files if not np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))]
    print("seeded training steps:", len(a.files), "arrays,", len(bad), "differ", bad[:10])
    eq = True
    if logits:
        la, lb = np.load(logits[0]), np.load(logits[1])
        eq = la.shape == lb.shape and np.array_equal(la.view(np.uint32), lb.view(np.uint32))
        print("bench logits", la.shape, "bit-equal:", eq)
    return 1 if bad or not eq else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4:6] if len(sys.argv) >= 6 else None))
