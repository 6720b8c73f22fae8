"""One WakewordTrainer.step with its options composed, stage by stage, from the restatements every option already has.  numpy only.

Nothing is derived here: every function hands a stage's own input -- as the test read it back from the device -- to the module that owns
the rule (qat_ref / quant_ref, select_ref, loss_ref / mixup_ref / distill_ref, trainer_ref, average_ref, ledger_ref) and returns what
the stage must leave behind.  tests/test_gpu_step_composed.py checks the chain on the GPU, tests/test_host_step_composed.py holds this
module to its parts without one.

  quantised         the tensors forward and backward read under QAT: fake-quant weights, the master's own biases
  selection         scores, the kept rows and the device record of a mined step
  loss              loss, dlogits and the counters of the launch `step` chooses: plain / options / class probabilities / distillation
  masked            the gradients after the straight-through launch
  clip              the global norm and clip_grad_norm_'s coefficient over every parameter's gradient
  update            one Adam update of (p, m, v) from the values before the step
  average           the averaged weights over the snapshots the Adam launches left
  ledger            the ledger after one more batch
  expected_launches the ops entry points of one step, in order (INTEGRATION.md sections 3n, 3p, 3r, 3t and 3u; the docstring of `step`)

and the configurations, batch sizes and input recipes the two test files share."""
import numpy as np

import average_ref
import distill_ref
import ledger_ref
import loss_ref
import mixup_ref
import qat_ref
import quant_ref
import select_ref
import trainer_ref

BETAS, EPS = (0.9, 0.999), 1e-8                                # torch.optim.Adam's defaults, which the trainer keeps
WEIGHT_DECAY = 1e-5                                            # WakewordTrainer's

# ---- the shared plan -----------------------------------------------------------------------------------------------------------------
BATCHES = (19, 5, 19, 33)                                      # a full 16-clip head workgroup and a partial one; a shrink; the same again;
EXTRA_BATCH = 33                                               # past the capacity -- and once more at the new capacity
N_ENTRIES = 40
W_EPS = {"weight": (0.25, 4.0), "label_smoothing": 0.125}      # loss_ref.WEIGHTS[1], loss_ref.SMOOTHINGS[1]: exact in float32

# model, then what is switched on.  qat: None or the quantiser's clip mode; teacher: None, "fixed" (a WakewordModel) or "mean"
# (average.model); target: "labels" (int64, one -100), "probs" (float32 [B, 2]) or None (unlabelled); select: None or
# (keep, keep_class); ledger: None, "device" or "host" entries.  Every one is a combination the trainer accepts: select= goes with
# neither a teacher nor QAT.
CONFIGS = {
    "qat_all": dict(model="simple", qat="mse", calibrate=2, teacher="fixed", alpha=0.3, temperature=2.0, opts=W_EPS, target="probs",
                    select=None, norm=True, average=True, ledger="device"),
    "qat_mean_teacher": dict(model="full", qat="mse", calibrate="epoch", teacher="mean", alpha=0.5, temperature=2.0, opts=None,
                             target="labels", select=None, norm=True, average=True, ledger="device"),
    "unlabelled": dict(model="simple", qat="max", calibrate="epoch", teacher="fixed", alpha=0.5, temperature=2.0, opts=None, target=None,
                       select=None, norm=True, average=True, ledger="device"),
    "select_focal": dict(model="full", qat=None, calibrate=None, teacher=None, alpha=None, temperature=None, opts={"focal_gamma": 2.0},
                         target="labels", select=(0.4, 1), norm=True, average=True, ledger="host"),
    "select_soft": dict(model="simple", qat=None, calibrate=None, teacher=None, alpha=None, temperature=None, opts=W_EPS, target="probs",
                        select=(7, None), norm=True, average=True, ledger="device"),
}
BITS = 4
DECAY = 0.9


def rows_kept(keep, B):
    """mining.HardSelect.rows restated: min(keep, B) for a count, the fraction rounded up (at least one row) otherwise."""
    if isinstance(keep, int):
        return min(keep, B)
    return min(B, max(1, int(np.ceil(round(keep * B, 9)))))


def kept_of(config, B):
    return B if config["select"] is None else rows_kept(config["select"][0], B)


def calibrates(config, step_index):
    """Whether step `step_index` (from 0) of a run searches the clip indices anew: qat_calibrate = n does so every n steps, not at 0."""
    n = config["calibrate"]
    return config["qat"] == "mse" and isinstance(n, int) and step_index > 0 and step_index % n == 0


def ignored_row(B):
    """The row whose integer label is -100."""
    return B // 2


def entries_for(B, step_index):
    """int64 [B] in 0 .. N_ENTRIES: seeded, with row 1 naming row 0's entry again (one entry twice in a batch)."""
    e = np.random.default_rng(500 + 10 * step_index + B).permutation(N_ENTRIES)[:B].astype(np.int64)
    e[1] = e[0]
    return e


def soft_targets(B, step_index):
    """mixup_ref.soft_inputs' probability rows: general, un-normalised, exact one-hot, one tie."""
    return mixup_ref.soft_inputs(B, seed=4000 + 10 * step_index + B)[1]


# ---- 1: the quantiser ------------------------------------------------------------------------------------------------------------------
def quantised(master, clip_idx, bits, per_channel=True):
    """master {name: float32 array} as it was before the step; clip_idx {name: uint8 [rows]} as the quantiser holds them, or None
    under clip="max" -> (read {name: what forward and backward read}, scale {name: float32 [rows]} of the quantised names).  Tensors
    of fewer than two dimensions (the biases) are the master's own."""
    read, scale = {}, {}
    for k, w in master.items():
        w = np.asarray(w, np.float32)
        if w.ndim < 2:
            read[k] = w.copy()
            continue
        r = quant_ref.quantize(w, bits, per_channel) if clip_idx is None else qat_ref.quantize_clip(w, clip_idx[k], bits, per_channel)
        read[k], scale[k] = r["deq"], r["scale"]
    return read, scale


# ---- 2: the selection ------------------------------------------------------------------------------------------------------------------
def is_plain(opts):
    """Whether ops.loss_opts makes None of these keywords: every option at its default, the plain ww_ce_loss_f32 rule."""
    o = dict(opts or {})
    return (o.get("weight") is None and o.get("label_smoothing", 0.0) == 0.0 and o.get("ignore_index", -100) == -100
            and o.get("reduction", "mean") == "mean" and o.get("focal_gamma") is None)


def selection(score_logits, targets, opts, keep, keep_class, scores=None):
    """The scoring pass's logits [B, 2] and the targets the rule ranks by -> dict(loss: the float64 per-clip losses, rank, bound: the
    absolute error a device score may have, sel: the kept rows, stats: one call's record).  `scores`: the device's own float64 scores;
    with them `sel` and `stats` are EXACTLY the order over those (the kernel ranks what it emitted), without them over `loss`."""
    o = None if is_plain(opts) else dict(opts)
    li, counting, cls = select_ref.losses(score_logits, targets, o)
    rank = select_ref.ranks(score_logits, li, counting, cls, keep_class)
    used = select_ref.scores_of(li, rank) if scores is None else np.asarray(scores, np.float64)
    sel = select_ref.select(used, rank, keep)
    return {"loss": li, "rank": rank, "bound": select_ref.bound(score_logits, (o or {}).get("weight") or (1.0, 1.0)), "sel": sel,
            "stats": select_ref.stats(used, rank, counting, cls, sel)}


# ---- 5: the loss -----------------------------------------------------------------------------------------------------------------------
def loss(logits, teacher_logits, targets, opts, alpha=0.5, temperature=2.0):
    """The launch `step` chooses, restated: with teacher logits distill_ref.distill (targets int64, float32 [n, 2] or None); else
    mixup_ref.soft_loss for float32 targets, trainer_ref.ce when every option is at its default, loss_ref.loss otherwise.  Returns
    dict(kind, loss, dlogits, want: the owning module's own result, train_stats, distill_stats or None); the two records hold what ONE
    step adds, `loss_sum` and the two float sums left out."""
    z = np.asarray(logits)
    n = z.shape[0]
    o = dict(opts or {})
    nonfinite = int((~np.isfinite(z.astype(np.float64)).all(axis=1)).sum())
    if teacher_logits is not None:
        if targets is None:
            o = {"reduction": o.get("reduction", "mean")}                              # an unlabelled batch reads the reduction alone
        w = distill_ref.distill(z, teacher_logits, targets, alpha, temperature, **o)
        return {"kind": "distill", "loss": w["loss"], "dlogits": w["dlogits"], "want": w, "train_stats": dict(w["stats"], batches=1),
                "distill_stats": dict(w["dstats"], batches=1)}
    t = np.asarray(targets)
    if t.dtype.kind == "f":
        w = mixup_ref.soft_loss(z, t, o.get("weight") or (1.0, 1.0), o.get("label_smoothing", 0.0), o.get("reduction", "mean"))
        kind = "soft"
    elif is_plain(o):
        l64, d64, correct = trainer_ref.ce(z, t)
        bad = int((~((t == 0) | (t == 1))).sum())
        w = {"loss": l64, "dlogits": d64, "correct": correct, "bad": bad, "denom": float(n), "max_w": 1.0, "counted": n - bad}
        kind = "plain"
    else:
        w = loss_ref.loss(z, t, o.get("weight") or (1.0, 1.0), o.get("label_smoothing", 0.0), o.get("ignore_index", -100),
                          o.get("reduction", "mean"), o.get("focal_gamma"))
        kind = "focal" if o.get("focal_gamma") is not None else "labels"
    return {"kind": kind, "loss": w["loss"], "dlogits": w["dlogits"], "want": w, "distill_stats": None,
            "train_stats": {"correct": w["correct"], "total": n, "batches": 1, "bad_labels": w["bad"], "nonfinite": nonfinite}}


# ---- 6: the straight-through mask ------------------------------------------------------------------------------------------------------
def masked(master, scale, grads, bits, per_channel=True):
    """grads {name: float32 array} as the backward left them -> the same with +0.0 where the clamp moved the master weight, for the
    names `scale` holds (clip="mse": the quantised tensors; an empty dict masks nothing)."""
    return {k: qat_ref.ste(np.asarray(master[k], np.float32), scale[k], g, bits, per_channel) if k in scale else np.array(g, np.float32, copy=True)
            for k, g in grads.items()}


# ---- 7: the norm -----------------------------------------------------------------------------------------------------------------------
def clip(grads, max_norm):
    """grads {parameter name: array} over EVERY parameter: the gradient buffer the two biases of an LSTM layer share is listed under
    both names and so counts twice, as clip_grad_norm_ counts it and WakewordTrainer._norm_step documents.  -> (norm, scale)."""
    return trainer_ref.clip(list(grads.values()), max_norm)


# ---- 8: Adam and the average -----------------------------------------------------------------------------------------------------------
def update(state, grads, scale, step, lr, weight_decay=WEIGHT_DECAY):
    """state {"p", "m", "v": {name: array}, "gmax"} before the step -> the same after one update (trainer_ref.adam_step per tensor),
    `gmax` raised to the largest |g'| met; the inputs are not touched."""
    out = {"p": {}, "m": {}, "v": {}, "gmax": float(state.get("gmax", 0.0))}
    for k in state["p"]:
        out["p"][k], out["m"][k], out["v"][k], g1 = trainer_ref.adam_step(state["p"][k], grads[k], state["m"][k], state["v"][k], lr, BETAS[0], BETAS[1],
                                                                           EPS, weight_decay, step, scale)
        out["gmax"] = max(out["gmax"], float(np.abs(g1).max()))
    return out


def average_weights(n_updates, decay=DECAY):
    """The weights of the first `n_updates` updates of an EMA without warmup (average.update_weight): 1, then 1 - decay."""
    return [1.0 if n == 0 else 1.0 - decay for n in range(n_updates)]


def average(snaps, weights):
    return average_ref.recursion(snaps, weights)


# ---- 9: the ledger ---------------------------------------------------------------------------------------------------------------------
def ledger(record, entries, logits, labels, epoch):
    """One more batch on a ledger_ref.RefLedger (made by `new_ledger`); returns it."""
    record.update(np.asarray(logits, np.float32), labels, entries, epoch)
    return record


def new_ledger(n_entries=N_ENTRIES):
    return ledger_ref.RefLedger(n_entries)


# ---- the launches ----------------------------------------------------------------------------------------------------------------------
LAUNCHES = ("quantize_weights_launch", "quantize_weights_clip_launch", "quant_clip_search_launch", "train_forward_into", "hard_select_into",
            "select_rows_into", "model_forward_into", "ce_loss_into", "soft_ce_loss_into", "distill_loss_into", "train_backward_into",
            "quant_ste_launch", "grad_norm_launch", "adam_launch", "adam_average_launch", "weight_average_launch", "clip_ledger_update_into")


def expected_launches(config, mined=None, calibrating=False):
    """The ops entry points one step of `config` calls, in order.  Written out from the text, not read from the code:
      3t  the quantiser first, ONE launch (the search in front of it on a calibrating step); forward and backward; under clip="mse" ONE
          straight-through launch after the backward and before the norm; then the norm and Adam
      3r  a mined step scores all rows (a forward), ranks them (one launch) and gathers (one launch) before the step as it always was
      3p  the teacher's eval forward after the student's, then ONE distillation launch in the loss's place
      3n  class-probability targets: the soft cross-entropy in the loss's place
      3o  an every="step" average rides in the Adam launch: adam_average_launch in adam_launch's place (both models fit one table)
      3m  the ledger's launch last, after the optimiser's
    `mined`: whether the step's k = rows(B) is below B (default: the configuration has a rule)."""
    mined = config["select"] is not None if mined is None else mined
    out = []
    if config["qat"] == "mse":
        out += ["quant_clip_search_launch"] if calibrating else []
        out += ["quantize_weights_clip_launch"]
    elif config["qat"] == "max":
        out += ["quantize_weights_launch"]
    if mined:
        out += ["train_forward_into", "hard_select_into", "select_rows_into"]
    out += ["train_forward_into"]
    if config["teacher"] is not None:
        out += ["model_forward_into", "distill_loss_into"]
    else:
        out += ["soft_ce_loss_into" if config["target"] == "probs" else "ce_loss_into"]
    out += ["train_backward_into"]
    if config["qat"] == "mse":
        out += ["quant_ste_launch"]
    if config["norm"]:
        out += ["grad_norm_launch"]
    out += ["adam_average_launch" if config["average"] else "adam_launch"]
    if config["ledger"] is not None:
        out += ["clip_ledger_update_into"]
    return out


def single(**on):
    """A configuration with everything off but `on`."""
    base = dict(model="simple", qat=None, calibrate=None, teacher=None, alpha=None, temperature=None, opts=None, target="labels", select=None,
                norm=False, average=False, ledger=None)
    base.update(on)
    return base
