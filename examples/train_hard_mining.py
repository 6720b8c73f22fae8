#!/usr/bin/env python3
"""Online hard example mining on a ClipBank: the training files are decoded once onto the GPU, the loader
yields candidate batches of 4096 clips, and every step trains on the quarter of them the model currently gets most wrong -- every
wake-word clip first (`keep_class=1`), then the hardest negatives -- chosen by ww_hard_select_f32 and gathered by ww_select_rows_f32
inside WakewordTrainer.step, without a wait on the device.  After each epoch the script prints what the selection did: the share of the
candidates that was trained on, the positives among candidates and kept rows, and the loss the last kept row had.

    PYTHONPATH=. python examples/train_hard_mining.py [--epochs 10] [--data DIR] [--batch-size 4096] [--keep 0.25] [--no-keep-positives]
                                                       [--class-weights balanced]

The epoch's loss and accuracy are over the KEPT rows, so they are harder than the batch's: compare runs by the validation figures.
"""
import argparse
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from train_from_files import split  # noqa: E402
from wakeword_jupyterlab_amd import (AudioProcessor, DataLoader, HardSelect, SimpleWakewordModel, TrainingConfig, WakewordDataset,  # noqa: E402
                                     WakewordTrainer, balanced_class_weights)
from wakeword_jupyterlab_amd.synth import create_sample_data  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--data", default=".")
    ap.add_argument("--batch-size", type=int, default=4096, help="candidate rows per step (up to 65536)")
    ap.add_argument("--keep", type=float, default=0.25, help="fraction of every batch that is trained on, in (0, 1]")
    ap.add_argument("--no-keep-positives", action="store_true", help="rank wake-word clips by loss like the rest (default: keep them all)")
    ap.add_argument("--class-weights", default=None, choices=("balanced",), help="weigh the loss -- and with it the ranking -- by class")
    a = ap.parse_args()
    device = torch.device("cuda")
    wdir, ndir = os.path.join(a.data, "wakeword_data"), os.path.join(a.data, "negative_data")
    if not os.path.exists(wdir) or len(os.listdir(wdir)) == 0:
        create_sample_data(a.data)
    wake = [f for ext in ("*.wav", "*.flac") for f in glob.glob(os.path.join(wdir, ext))]
    neg = [f for ext in ("*.wav", "*.flac") for f in glob.glob(os.path.join(ndir, ext))]
    w_tr, w_va, _ = split(wake)
    n_tr, n_va, _ = split(neg)
    config = type("TrainingConfig", (TrainingConfig,), {"BATCH_SIZE": a.batch_size, "EPOCHS": a.epochs})
    processor = AudioProcessor()
    model = SimpleWakewordModel().to(device)
    bank = WakewordDataset(w_tr, n_tr, processor, augment=True).cache()           # every training file decoded once, onto the GPU
    print(bank)
    train_loader = DataLoader(bank, batch_size=config.BATCH_SIZE, shuffle=True, augment=True)
    val_loader = DataLoader(WakewordDataset(w_va, n_va, processor, augment=False).cache(), batch_size=config.BATCH_SIZE, shuffle=False)
    crit = None
    if a.class_weights == "balanced":
        crit = torch.nn.CrossEntropyLoss(weight=balanced_class_weights([0] * len(n_tr) + [1] * len(w_tr))).to(device)
    rule = HardSelect(a.keep, keep_class=None if a.no_keep_positives else 1)
    trainer = WakewordTrainer(model, device, config, checkpoint_path=os.path.join(a.data, "best_mined_model.pth"), criterion=crit, select=rule)
    print(f"Selection: {rule} -> {rule.rows(config.BATCH_SIZE)} of {config.BATCH_SIZE} rows per full batch")
    for epoch in range(config.EPOCHS):
        train_loss, train_acc = trainer.train_epoch(train_loader)
        val_loss, val_acc = trainer.validate(val_loader)
        r = trainer.select_report
        print(f"epoch {epoch + 1}: kept rows loss {train_loss:.4f} acc {train_acc:.2f}% | val loss {val_loss:.4f} acc {val_acc:.2f}%")
        if r["batches"]:
            print(f"   trained on {100 * r['kept_fraction']:.1f}% of {r['candidates']} candidates; positives {100 * r['candidate_positive_fraction']:.1f}% "
                  f"of the candidates, {100 * r['kept_positive_fraction']:.1f}% of the kept; unranked rows {r['unranked']} "
                  f"({r['kept_unranked']} kept); last threshold {r['threshold']:.4g}")
        else:
            print("   no batch was larger than the rows to keep: nothing was mined")
    torch.save({"model_state_dict": model.state_dict(), "device": str(device)}, os.path.join(a.data, "final_mined_model.pth"))


if __name__ == "__main__":
    main()
