#!/usr/bin/env python3
"""After training: turn the two-conv SimpleWakewordModel's float32 weights into the int8 weights a small device
stores, see what that costs, and write a package both sides can read.  The model is trained by the fused step with `quant=` and
`evaluate="quant"`, so every validation runs on the quantised weights and the checkpoint that is kept is the one that survives
quantisation; then the fake-quant model is evaluated like any model, at `--bits` and -- to see where it breaks -- at 6 and 4 bits.
`--clip mse` takes every row's scale from the clip with the smallest squared error; `--qat N` (section 3t) trains N more epochs THROUGH
the quantiser -- forward and backward on the fake-quant weights, Adam on the float32 ones -- and prints the quantised model's validation
loss before and after.

    PYTHONPATH=. python examples/quantize.py [--epochs 10] [--bits 8] [--per-tensor] [--clip mse] [--qat 5] [--data DIR] [--batch-size 16]
"""
import argparse
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from train_from_files import split  # noqa: E402
from wakeword_jupyterlab_amd import (AudioProcessor, DataLoader, SimpleWakewordModel, TrainingConfig, WakewordDataset, WakewordTrainer,  # noqa: E402
                                     WeightQuant, evaluate_report, load_quantized_package, save_quantized_package)
from wakeword_jupyterlab_amd.synth import create_sample_data  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=TrainingConfig.EPOCHS)
    ap.add_argument("--bits", type=int, default=8, help="2 .. 8; the values are stored as int8 either way")
    ap.add_argument("--per-tensor", action="store_true", help="one scale per tensor, not per output channel / row")
    ap.add_argument("--clip", choices=("max", "mse"), default="max", help="the scale rule: the row's largest element, or the best of 48 clips")
    ap.add_argument("--qat", type=int, default=0, metavar="EPOCHS", help="quantisation-aware epochs after the float32 training")
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
    bank = WakewordDataset(w_tr, n_tr, processor, augment=True).cache()
    train_loader = bank.loader(a.batch_size, shuffle=True, augment=True)
    val_loader = DataLoader(WakewordDataset(w_va, n_va, processor, augment=False).cache(), batch_size=a.batch_size, shuffle=False)

    # ---- 1. train with the validation on the quantised weights ----
    model = SimpleWakewordModel().to(device)
    quant = WeightQuant(model, bits=a.bits, per_channel=not a.per_tensor, clip=a.clip)
    trainer = WakewordTrainer(model, device, checkpoint_path=os.path.join(a.data, "best_wakeword_model.pth"), quant=quant, evaluate="quant")
    best = trainer.train(train_loader, val_loader, a.epochs)

    # ---- 2. the best checkpoint's integers, and what they cost ----
    ckpt = torch.load(os.path.join(a.data, "best_wakeword_model.pth"), weights_only=True)
    model.load_state_dict(ckpt["model_state_dict"])
    quant.calibrate()                                                             # = quant.load_state_dict(ckpt["quant_state_dict"])

    # ---- 2b. quantisation-aware epochs: the weights learn to survive the quantiser ----
    if a.qat > 0:
        qat = WakewordTrainer(model, device, checkpoint_path=os.path.join(a.data, "best_wakeword_model_qat.pth"), quant=quant, evaluate="quant",
                              qat=True)
        before = qat.validate(val_loader)
        best = qat.train(train_loader, val_loader, a.qat)
        ckpt = torch.load(os.path.join(a.data, "best_wakeword_model_qat.pth"), weights_only=True)
        model.load_state_dict(ckpt["model_state_dict"])
        quant.calibrate()
        after = qat.validate(val_loader)
        print(f"int{a.bits} weights, validation loss / accuracy: {before[0]:.4f} / {before[1]:.2f}% before, {after[0]:.4f} / {after[1]:.2f}% "
              f"after {a.qat} quantisation-aware epochs")
    print(quant.report())
    print("float32 model:")
    print(evaluate_report(model.eval(), val_loader).summary())
    print(f"int{a.bits} weights:")
    print(evaluate_report(quant.model, val_loader).summary())
    for bits in (6, 4):
        lower = WeightQuant(model, bits=bits, per_channel=not a.per_tensor, clip=a.clip)
        r = evaluate_report(lower.model, val_loader)
        print(f"int{bits} weights: accuracy {100.0 * r.accuracy:.2f}%  weights' SQNR {lower.report().totals['sqnr_db']:.1f} dB")

    # ---- 3. the package: float32 weights for the reference's loader, q and scale for the device ----
    path = os.path.join(a.data, "wakeword_deployment_int8.pth")
    save_quantized_package(quant, path, best_val_accuracy=best, epoch=ckpt["epoch"], device=device)
    on_cpu = SimpleWakewordModel()                                                # rebuilt from q * scale alone, no GPU needed
    st = load_quantized_package(path, on_cpu)["quantized"]
    same = all(torch.equal(p, q.cpu()) for p, q in zip(on_cpu.parameters(), quant.model.parameters()))
    print(f"{path}: {sum(v.numel() for v in st['q'].values()):,} int8 weights, {sum(v.numel() for v in st['scale'].values()):,} scales; "
          f"reloaded weights equal the evaluated ones: {same}")


if __name__ == "__main__":
    main()
