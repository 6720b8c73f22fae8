"""The bits of the three cross-entropy entry points against a record taken from a trusted build (tests/golden/loss_bits.json, written by
tests/golden/make_loss_bits.py, which also defines the cases): the gradient's sha256, the loss's 32-bit pattern and the six stats words
of every case, on tensors on the 16-byte grid and off it -- logits and gradient 4 bytes, labels 8 bytes, probabilities 4 bytes.

No tolerance: a refactor of the loss kernels must not move a bit.  The hashes depend on the ROCm device math library (exp, log and the
float64 division) as well as on this project's code: after a ROCm update that moves them, and after a deliberate change to the loss
arithmetic, regenerate the file with make_loss_bits.py from a commit whose loss code is trusted -- never from the code under test."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_spec = importlib.util.spec_from_file_location("make_loss_bits", os.path.join(GOLDEN, "make_loss_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def record():
    with open(os.path.join(GOLDEN, "loss_bits.json")) as f:
        return json.load(f)


def test_the_record_holds_exactly_the_generators_cases(record):
    assert len(record["commit"]) == 40 and len(record["ww_optim.hip"]) == 64
    assert list(record["cases"]) == [f"n={n} {tag}" for n, tag, *_ in gen.keys()]
    assert os.path.getsize(os.path.join(GOLDEN, "loss_bits.json")) <= 32 * 1024


@pytest.mark.parametrize("n", gen.SIZES)
def test_loss_bits_are_the_recorded_ones(record, n):
    for tag, kind, replace, opts in gen.CASES:
        key = f"n={n} {tag}"
        got = gen.measure(n, tag, kind, replace, opts, DEV)           # asserts aligned == off grid and the guard words itself
        want = record["cases"][key]
        assert got["inputs"] == want["inputs"], f"{key}: the INPUTS differ from the recorded ones (the generator or numpy changed, not the kernel)"
        for field in ("stats", "loss", "dlogits"):
            assert got[field] == want[field], f"{key}: {field} {got[field]} != recorded {want[field]} (build of {record['commit'][:12]})"
