#!/usr/bin/env python3
"""The reference's `main()` (wakeword_training_script.py:395-495) with its own training class: sample data -> file lists -> split ->
AudioProcessor / WakewordModel -> WakewordTrainer(model, device).train(train_loader, val_loader, epochs) -> best / final checkpoints.
The training files live in a ClipBank on the GPU and every batch runs forward, cross-entropy, backward and
Adam as HIP kernels without a wait on the device (section 3h); the epoch's loss and accuracy are read once per epoch.  It ends as the
notebook's evaluation cell does (cell 17): accuracy, weighted precision / recall / F1, the confusion matrix and the classification report
of the test set -- from counters kept on the device (section 3j) -- and, beyond the reference, the operating point at 0.8, AUC and EER.

    PYTHONPATH=. python examples/train_with_trainer.py [--epochs 10] [--data DIR] [--duration 1.0] [--background DIR] [--max-grad-norm 1.0]
                                                        [--spec-augment] [--monitor val_acc|val_f1|val_auc]
                                                        [--class-weights balanced|W0,W1] [--label-smoothing E] [--focal-gamma G]
                                                        [--positive-fraction F] [--mixup] [--ema DECAY]

Imbalanced data (section 3k): `--class-weights balanced` weighs the classes by the training split's counts, `--label-smoothing` and
`--focal-gamma` choose the loss of the fused step, `--positive-fraction 0.5` makes every training epoch half wake-word items.
`--mixup` (section 3n) mixes rows of every training batch on the GPU and trains on the class probabilities that result.
`--ema 0.999` (section 3o) keeps an exponential moving average of the weights inside the Adam launch; validation, the scheduler, the best
checkpoint, early stopping and the final test then follow the averaged model, which is also what `ema_wakeword_model.pth` holds.
"""
import argparse
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from train_from_files import split  # noqa: E402
from wakeword_jupyterlab_amd import (AudioConfig, AudioProcessor, DataLoader, FocalLoss, MixupConfig, SpecAugmentConfig,  # noqa: E402
                                     TrainingConfig, WakewordDataset, WakewordModel, WakewordTrainer, WeightAverage, balanced_class_weights)
from wakeword_jupyterlab_amd.synth import create_sample_data  # noqa: E402


def criterion(a, n_negative, n_positive):
    """The loss the flags name, or None for the trainer's default nn.CrossEntropyLoss()."""
    weight = None
    if a.class_weights == "balanced":
        weight = balanced_class_weights([0] * n_negative + [1] * n_positive)
    elif a.class_weights is not None:
        weight = torch.tensor([float(v) for v in a.class_weights.split(",")])
    if a.focal_gamma is not None:
        if a.label_smoothing:
            raise SystemExit("--focal-gamma and --label-smoothing exclude one another")
        return FocalLoss(a.focal_gamma, weight=weight)
    if weight is None and not a.label_smoothing:
        return None
    return torch.nn.CrossEntropyLoss(weight=weight, label_smoothing=a.label_smoothing)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=TrainingConfig.EPOCHS)
    ap.add_argument("--data", default=".")
    ap.add_argument("--lr", type=float, default=TrainingConfig.LEARNING_RATE)
    ap.add_argument("--batch-size", type=int, default=TrainingConfig.BATCH_SIZE)
    ap.add_argument("--duration", type=float, default=AudioConfig.DURATION, help="clip length in seconds, 0.25 .. 1.0")
    ap.add_argument("--background", default=None, help="directory of background noise files (WAV / FLAC) mixed into the training clips")
    ap.add_argument("--max-grad-norm", type=float, default=None, help="clip the global gradient norm after the backward (default: off)")
    ap.add_argument("--spec-augment", action="store_true", help="mask blocks of mel bins and frames of every training batch (SpecAugment)")
    ap.add_argument("--mixup", action="store_true",
                    help="mix rows of every training batch and train on class probabilities (mixup; excludes --focal-gamma)")
    ap.add_argument("--monitor", default="val_acc", choices=("val_acc", "val_f1", "val_auc"),
                    help="what the scheduler, the best checkpoint and early stopping follow (default: the reference's validation accuracy)")
    ap.add_argument("--class-weights", default=None, metavar="balanced|W0,W1",
                    help="class weights of the loss: 'balanced' (n / (2 n_c) over the training split) or two numbers, negative then wake word")
    ap.add_argument("--label-smoothing", type=float, default=0.0, help="label smoothing of the cross-entropy, in [0, 1]")
    ap.add_argument("--focal-gamma", type=float, default=None, help="train with the focal loss of this gamma instead of cross-entropy")
    ap.add_argument("--positive-fraction", type=float, default=None,
                    help="share of wake-word items in every training epoch, in (0, 1) (default: the files as they are)")
    ap.add_argument("--ema", type=float, default=None, metavar="DECAY",
                    help="keep an exponential moving average of the weights with this decay (with warmup) and evaluate it (default: off)")
    a = ap.parse_args()
    device = torch.device("cuda")
    print(f"Using device: {device} ({torch.cuda.get_device_name(0)})")
    wdir, ndir = os.path.join(a.data, "wakeword_data"), os.path.join(a.data, "negative_data")
    if not os.path.exists(wdir) or len(os.listdir(wdir)) == 0:
        create_sample_data(a.data)
    wake = [f for ext in ("*.wav", "*.flac") for f in glob.glob(os.path.join(wdir, ext))]
    neg = [f for ext in ("*.wav", "*.flac") for f in glob.glob(os.path.join(ndir, ext))]
    print(f"Wakeword files: {len(wake)}   Negative files: {len(neg)}")
    w_tr, w_va, w_te = split(wake)
    n_tr, n_va, n_te = split(neg)
    audio_config = type("AudioConfig", (AudioConfig,), {"DURATION": a.duration})
    config = type("TrainingConfig", (TrainingConfig,), {"LEARNING_RATE": a.lr, "BATCH_SIZE": a.batch_size, "EPOCHS": a.epochs})
    processor = AudioProcessor(audio_config)
    if a.background:
        processor.set_background_noise(a.background)
    if a.spec_augment:
        processor.set_spec_augment(SpecAugmentConfig)                             # training loader only: the others run with augment=False
    if a.mixup:
        if a.focal_gamma is not None:
            raise SystemExit("--mixup and --focal-gamma exclude one another: the focal loss takes integer labels")
        processor.set_mixup(MixupConfig)                                          # training loader only, after SpecAugment
    model = WakewordModel(audio_config=audio_config).to(device)
    print(f"Parameters: {sum(p.numel() for p in model.parameters()):,}")
    bank = WakewordDataset(w_tr, n_tr, processor, augment=True).cache()           # every training file decoded once, onto the GPU
    print(bank)
    train_loader = DataLoader(bank, batch_size=config.BATCH_SIZE, shuffle=True, augment=True, positive_fraction=a.positive_fraction)
    val_loader = DataLoader(WakewordDataset(w_va, n_va, processor, augment=False).cache(), batch_size=config.BATCH_SIZE, shuffle=False)
    test_loader = DataLoader(WakewordDataset(w_te, n_te, processor, augment=False).cache(), batch_size=config.BATCH_SIZE, shuffle=False)
    crit = criterion(a, len(n_tr), len(w_tr))
    ema = WeightAverage(model, mode="ema", decay=a.ema, warmup=True) if a.ema is not None else None
    trainer = WakewordTrainer(model, device, config, checkpoint_path=os.path.join(a.data, "best_wakeword_model.pth"),
                              max_grad_norm=a.max_grad_norm, monitor=a.monitor, thresholds=(0.8,), criterion=crit.to(device) if crit is not None else None,
                              average=ema, evaluate="average" if ema is not None else "model")
    print(f"Criterion: {trainer.criterion}")
    best = trainer.train(train_loader, val_loader, config.EPOCHS)
    _, test_acc = trainer.validate(test_loader)
    print(f"Best validation accuracy: {best:.2f}%   Test accuracy: {test_acc:.2f}%")
    report = trainer.val_report                                                   # of the validate just above: the test set, read once
    s = report.summary()
    print("\nTest Set Performance:")
    print(f"   Accuracy: {s['accuracy']:.4f}\n   Precision: {s['precision']:.4f}\n   Recall: {s['recall']:.4f}\n   F1-Score: {s['f1']:.4f}")
    print(f"\nConfusion Matrix (rows: actual Negative, Wakeword; columns: predicted):\n{report.confusion}")
    print("\nClassification Report:")
    print(report.classification_report(target_names=("Negative", "Wakeword")))
    at = report.at(0.8)
    print(f"At threshold 0.80: {at['tp']} detected, {at['fn']} missed, {at['fp']} false accepts of {at['fp'] + at['tn']} negatives "
          f"(FPR {at['fpr']:.4f}, FNR {at['fnr']:.4f})")
    if report.support.min() > 0:
        print(f"ROC AUC: {report.auc:.4f} (+- {report.auc_bound:.1e} from binning)   EER: {report.eer:.4f}   "
              f"threshold for FPR <= 1 %: {report.threshold_for(0.01):.4f}")
    torch.save({"model_state_dict": model.state_dict(), "best_val_acc": best, "device": str(device)},
               os.path.join(a.data, "final_wakeword_model.pth"))
    if ema is not None:
        torch.save({"model_state_dict": ema.model.state_dict(), "best_val_acc": best, "n_averaged": ema.n_averaged, "device": str(device)},
                   os.path.join(a.data, "ema_wakeword_model.pth"))


if __name__ == "__main__":
    main()
