"""tests/step_ref.py held to its parts without a GPU: with every option off it IS trainer_ref.ce plus trainer_ref.adam_step, every stage
hands its input to the module that owns the rule, the launch lists of the single-option configurations are the ones the options' own
GPU tests assert, and the input recipes of tests/test_gpu_step_composed.py meet the conditions that depend on the inputs alone."""
import numpy as np
import pytest

import distill_ref
import loss_ref
import mixup_ref
import qat_ref
import quant_ref
import step_ref as sr
import trainer_ref
import wakeword_jupyterlab_amd as pkg
from wakeword_jupyterlab_amd.average import update_weight


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- every option off -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 19, 33])
def test_with_every_option_off_the_step_is_ce_and_adam_bit_for_bit(n):
    z, y = trainer_ref.ce_inputs(n, seed=n)
    got = sr.loss(z, None, y, None)
    l64, d64, correct = trainer_ref.ce(z, y)
    assert got["kind"] == "plain" and got["loss"] == l64 and _same(got["dlogits"], d64) and got["distill_stats"] is None
    assert got["train_stats"] == {"correct": correct, "total": n, "batches": 1, "bad_labels": 0, "nonfinite": 0}
    p0, gs = trainer_ref.adam_inputs(257, seed=n, steps=2)
    state = {"p": {"w": p0}, "m": {"w": np.zeros(257)}, "v": {"w": np.zeros(257)}, "gmax": 0.0}
    want = (p0, np.zeros(257), np.zeros(257))
    for t in range(2):
        grads = {"w": gs[t]}
        assert all(_same(a, b) for a, b in zip(sr.masked({"w": p0}, {}, grads, sr.BITS).values(), grads.values()))        # no quantiser: no mask
        state = sr.update(state, grads, 1.0, t + 1, lr=1e-3)
        want = trainer_ref.adam_step(want[0], gs[t], want[1], want[2], 1e-3, 0.9, 0.999, 1e-8, 1e-5, t + 1)[:3]
        assert all(_same(state[r]["w"], w) for r, w in zip("pmv", want))
    assert sr.kept_of(sr.single(), n) == n and not sr.calibrates(sr.single(), 2)
    assert sr.expected_launches(sr.single()) == ["train_forward_into", "ce_loss_into", "train_backward_into", "adam_launch"]


def test_a_minus_100_label_follows_the_rule_of_the_launch():
    """The default criterion alone counts -100 as a bad label; with any option, or beside a teacher, it is ignored."""
    z, y = trainer_ref.ce_inputs(19, seed=3)
    y = y.copy()
    y[sr.ignored_row(19)] = -100
    assert sr.loss(z, None, y, None)["train_stats"]["bad_labels"] == 1
    assert sr.loss(z, None, y, {"focal_gamma": 2.0})["train_stats"]["bad_labels"] == 0
    with_teacher = sr.loss(z, z[::-1].copy(), y, None, 0.5, 2.0)
    assert with_teacher["train_stats"]["bad_labels"] == 0 and with_teacher["distill_stats"]["hard_rows"] == 18 and with_teacher["distill_stats"]["kd_rows"] == 19


# ---- every stage is its owner's restatement ---------------------------------------------------------------------------------------------
def test_the_loss_dispatches_as_the_step_does():
    z, zt, y, t = distill_ref.inputs(33, nonfinite_teacher=False)
    y = np.where((y == 0) | (y == 1), y, -100)
    t[5] = (0.25, 0.75)
    o = sr.W_EPS
    focal = sr.loss(z, None, y, {"focal_gamma": 2.0})
    assert focal["kind"] == "focal" and _same(focal["dlogits"], loss_ref.loss(z, y, focal_gamma=2.0)["dlogits"])
    assert focal["train_stats"]["correct"] == loss_ref.loss(z, y, focal_gamma=2.0)["correct"]
    soft = sr.loss(z, None, t, o)
    want = mixup_ref.soft_loss(z, t, o["weight"], o["label_smoothing"])
    assert soft["kind"] == "soft" and soft["loss"] == want["loss"] and _same(soft["dlogits"], want["dlogits"])
    for target, opts in ((t, o), (y, None), (None, o)):
        got = sr.loss(z, zt, target, opts, 0.3, 2.0)
        kw = {} if opts is None else dict(opts) if target is not None else {}
        want = distill_ref.distill(z, zt, target, 0.3, 2.0, **kw)
        assert got["kind"] == "distill" and got["loss"] == want["loss"] and _same(got["dlogits"], want["dlogits"])
        assert got["train_stats"] == dict(want["stats"], batches=1) and got["distill_stats"] == dict(want["dstats"], batches=1)


def test_quantised_masked_and_clip_are_their_owners():
    rng = np.random.default_rng(5)
    master = {"conv.weight": (0.05 * rng.standard_normal((6, 4, 3, 3))).astype(np.float32), "conv.bias": rng.standard_normal(6).astype(np.float32),
              "fc.weight": (0.05 * rng.standard_normal((2, 65))).astype(np.float32)}
    clips = {"conv.weight": np.array([0, 3, 47, 9, 20, 1], np.uint8), "fc.weight": np.array([12, 30], np.uint8)}
    read, scale = sr.quantised(master, clips, 4)
    assert sorted(scale) == ["conv.weight", "fc.weight"] and _same(read["conv.bias"], master["conv.bias"])
    for k in scale:
        want = qat_ref.quantize_clip(master[k], clips[k], 4)
        assert _same(read[k], want["deq"]) and _same(scale[k], want["scale"]) and want["sat"].sum() > 0
    plain, pscale = sr.quantised(master, None, 4)
    assert _same(plain["fc.weight"], quant_ref.quantize(master["fc.weight"], 4)["deq"]) and _same(pscale["fc.weight"], quant_ref.quantize(master["fc.weight"], 4)["scale"])
    grads = {k: rng.standard_normal(v.shape).astype(np.float32) for k, v in master.items()}
    cut = sr.masked(master, scale, grads, 4)
    assert _same(cut["conv.bias"], grads["conv.bias"]) and _same(cut["fc.weight"], qat_ref.ste(master["fc.weight"], scale["fc.weight"], grads["fc.weight"], 4))
    assert not _same(cut["conv.weight"], grads["conv.weight"])
    # a gradient listed under two names counts twice, and masking changes the norm
    shared = dict(grads, **{"conv.bias_again": grads["conv.bias"]})
    n1, _ = sr.clip(grads, 1.0)
    n2, s2 = sr.clip(shared, 1.0)
    assert n2 == trainer_ref.clip(list(grads.values()) + [grads["conv.bias"]], 1.0)[0] and n2 > n1 and s2 == min(1.0, 1.0 / (n2 + 1e-6))
    assert sr.clip(cut, 1.0)[0] < n1


# ---- the launch lists -------------------------------------------------------------------------------------------------------------------
def test_single_option_launch_lists_are_the_ones_the_options_own_gpu_tests_assert():
    plain = ["train_forward_into", "ce_loss_into", "train_backward_into", "adam_launch"]
    # tests/test_gpu_qat.py, test_qat_step_launches_waits_and_allocations
    assert sr.expected_launches(sr.single(qat="max")) == ["quantize_weights_launch"] + plain
    assert sr.expected_launches(sr.single(qat="mse")) == ["quantize_weights_clip_launch"] + plain[:3] + ["quant_ste_launch", "adam_launch"]
    # tests/test_gpu_average.py, test_average_changes_nothing_else_and_adds_no_launch: the plain list with the averaged launch in Adam's place
    avg = sr.expected_launches(sr.single(average=True))
    assert [c.replace("adam_average_launch", "adam_launch") for c in avg] == plain and avg.count("adam_average_launch") == 1
    # tests/test_gpu_select.py, test_mined_step_equals_a_twin_driven_by_hand: the dropout-free forward, the selection, then a plain step
    mined = sr.expected_launches(sr.single(select=(5, None)))
    assert mined == ["train_forward_into", "hard_select_into", "select_rows_into"] + plain
    assert sr.expected_launches(sr.single(select=(5, None)), mined=False) == plain
    # tests/test_gpu_quant.py NAMES and tests/test_gpu_qat.py NAMES are subsets of what is recorded
    assert set(sum((sr.expected_launches(c, calibrating=True) for c in sr.CONFIGS.values()), [])) <= set(sr.LAUNCHES)
    full = sr.expected_launches(sr.CONFIGS["qat_all"], calibrating=True)
    assert full == ["quant_clip_search_launch", "quantize_weights_clip_launch", "train_forward_into", "model_forward_into", "distill_loss_into",
                    "train_backward_into", "quant_ste_launch", "grad_norm_launch", "adam_average_launch", "clip_ledger_update_into"]


# ---- the recipes ------------------------------------------------------------------------------------------------------------------------
def test_configurations_are_legal_and_the_batches_cross_the_edges():
    assert sr.BATCHES == (19, 5, 19, 33) and sr.EXTRA_BATCH == 33 and sorted(sr.CONFIGS) == sorted(["qat_all", "qat_mean_teacher", "unlabelled",
                                                                                                     "select_focal", "select_soft"])
    for name, c in sr.CONFIGS.items():
        if c["select"] is not None:                               # the trainer's refusals
            assert c["teacher"] is None and c["qat"] is None, name
            rule = pkg.HardSelect(*c["select"])
            assert all(rule.rows(B) == sr.kept_of(c, B) for B in range(1, 40)), name
        if c["target"] == "probs":
            assert (c["opts"] or {}).get("focal_gamma") is None, name
        if c["target"] is None:
            assert c["teacher"] is not None, name
        assert c["teacher"] != "mean" or c["average"], name
    focal, soft = sr.CONFIGS["select_focal"], sr.CONFIGS["select_soft"]
    assert all(0 < sr.kept_of(focal, B) < B for B in sr.BATCHES) and focal["select"][1] == 1                # every step mines
    assert sr.kept_of(soft, 5) >= 5 and all(0 < sr.kept_of(soft, B) < B for B in (19, 33))                 # the B = 5 step does not
    q = sr.CONFIGS["qat_all"]
    assert [sr.calibrates(q, i) for i in range(5)] == [False, False, True, False, True] and q["calibrate"] == 2
    assert not any(sr.calibrates(sr.CONFIGS[n], i) for n in ("qat_mean_teacher", "unlabelled") for i in range(5))


def test_entries_labels_and_probability_targets_meet_their_conditions():
    for i, B in enumerate(sr.BATCHES + (sr.EXTRA_BATCH,)):
        e = sr.entries_for(B, i)
        assert e.dtype == np.int64 and e.shape == (B,) and e.min() >= 0 and e.max() < sr.N_ENTRIES
        assert e[0] == e[1] and len(set(e.tolist())) == B - 1                                  # one entry twice, no other repeat
        assert 0 <= sr.ignored_row(B) < B and sr.ignored_row(B) > 1                            # not one of the duplicated rows
        t = sr.soft_targets(B, i)
        assert t.dtype == np.float32 and t.shape == (B, 2) and np.isfinite(t).all() and (t >= 0).all()          # every row counts
        assert tuple(t[0]) == (0.5, 0.5) and np.any((t == 1.0).any(axis=1)) and len({tuple(r) for r in t.tolist()}) > 2
    assert not _same(sr.soft_targets(19, 0), sr.soft_targets(19, 2))                           # the two B = 19 steps differ
    assert sr.average_weights(4) == [update_weight(n, "ema", sr.DECAY) for n in range(4)] and sr.average_weights(1) == [1.0]
