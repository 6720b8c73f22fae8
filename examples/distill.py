#!/usr/bin/env python3
"""The last step of the wake-word workflow: train the three-conv WakewordModel, then teach the two-conv
SimpleWakewordModel -- the one that fits a small device -- to reproduce it.  The training files live in a ClipBank on the GPU; the teacher
is trained by the fused step as in examples/train_with_trainer.py, and the student by the same step with `teacher=`: the teacher's eval
forward on every batch and ONE loss launch for (1 - alpha) * cross-entropy + alpha * T^2 * KD.  `--unlabelled` then runs epochs in which
the labels are withheld (`step(data, None)`: the loss is T^2 * KD alone), as one would on recordings nobody has labelled.

    PYTHONPATH=. python examples/distill.py [--teacher-epochs 10] [--epochs 10] [--alpha 0.5] [--temperature 2.0] [--unlabelled 2]
                                            [--data DIR] [--batch-size 16]
"""
import argparse
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from train_from_files import split  # noqa: E402
from wakeword_jupyterlab_amd import (AudioProcessor, DataLoader, SimpleWakewordModel, TrainingConfig, WakewordDataset,  # noqa: E402
                                     WakewordModel, WakewordTrainer)
from wakeword_jupyterlab_amd.synth import create_sample_data  # noqa: E402


def without_labels(loader):
    """The loader's batches with the labels withheld: what a loader over unlabelled recordings yields."""
    for data, _ in loader:
        yield data, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--teacher-epochs", type=int, default=TrainingConfig.EPOCHS)
    ap.add_argument("--epochs", type=int, default=TrainingConfig.EPOCHS, help="distillation epochs with labels")
    ap.add_argument("--unlabelled", type=int, default=0, help="further epochs with the labels withheld (the teacher term alone)")
    ap.add_argument("--alpha", type=float, default=0.5, help="weight of the teacher term, in [0, 1]")
    ap.add_argument("--temperature", type=float, default=2.0, help="softmax temperature of the teacher term")
    ap.add_argument("--data", default=".")
    ap.add_argument("--batch-size", type=int, default=TrainingConfig.BATCH_SIZE)
    a = ap.parse_args()
    device = torch.device("cuda")
    wdir, ndir = os.path.join(a.data, "wakeword_data"), os.path.join(a.data, "negative_data")
    if not os.path.exists(wdir) or len(os.listdir(wdir)) == 0:
        create_sample_data(a.data)
    wake = [f for ext in ("*.wav", "*.flac") for f in glob.glob(os.path.join(wdir, ext))]
    neg = [f for ext in ("*.wav", "*.flac") for f in glob.glob(os.path.join(ndir, ext))]
    w_tr, w_va, _ = split(wake)
    n_tr, n_va, _ = split(neg)
    processor = AudioProcessor()
    bank = WakewordDataset(w_tr, n_tr, processor, augment=True).cache()           # every training file decoded once, onto the GPU
    print(bank)
    train_loader = bank.loader(a.batch_size, shuffle=True, augment=True)
    val_loader = DataLoader(WakewordDataset(w_va, n_va, processor, augment=False).cache(), batch_size=a.batch_size, shuffle=False)

    # ---- 1. the teacher: the model one trains for accuracy ----
    teacher = WakewordModel().to(device)
    WakewordTrainer(teacher, device, checkpoint_path=os.path.join(a.data, "teacher_wakeword_model.pth")).train(train_loader, val_loader,
                                                                                                               a.teacher_epochs)
    teacher.eval()                                                                # a teacher in train mode is refused
    for p in teacher.parameters():
        p.requires_grad_(False)

    # ---- 2. the student: every batch also sees the teacher's logits ----
    student = SimpleWakewordModel().to(device)
    print(f"teacher {sum(p.numel() for p in teacher.parameters()):,} parameters -> student {sum(p.numel() for p in student.parameters()):,}")
    trainer = WakewordTrainer(student, device, checkpoint_path=os.path.join(a.data, "student_wakeword_model.pth"), teacher=teacher,
                              distill_alpha=a.alpha, distill_temperature=a.temperature)
    for epoch in range(a.epochs):
        loss, acc = trainer.train_epoch(train_loader)
        r = trainer.distill_report                                                # read with the epoch's loss, in the same copy
        val_loss, val_acc = trainer.validate(val_loader)                          # plain cross-entropy on the labels, as without a teacher
        print(f"Epoch {epoch + 1}/{a.epochs}  loss {loss:.4f} (hard {r['hard_loss']:.4f}, KD {r['kd_loss']:.4f})  acc {acc:.2f}%  "
              f"agrees with the teacher on {r['agreement']:.2f}%  teacher acc {r['teacher_accuracy']:.2f}%  val acc {val_acc:.2f}%")

    # ---- 3. recordings without labels: the teacher term alone ----
    for epoch in range(a.unlabelled):
        loss, _ = trainer.train_epoch(without_labels(train_loader))
        r = trainer.distill_report
        _, val_acc = trainer.validate(val_loader)
        print(f"Unlabelled epoch {epoch + 1}/{a.unlabelled}  T^2 KD {loss:.4f}  agrees with the teacher on {r['agreement']:.2f}%  "
              f"val acc {val_acc:.2f}%")
    torch.save({"model_state_dict": student.state_dict(), "device": str(device)}, os.path.join(a.data, "student_final_wakeword_model.pth"))


if __name__ == "__main__":
    main()
