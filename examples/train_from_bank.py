#!/usr/bin/env python3
"""The flow of examples/train_from_files.py with the training files kept in device memory: `train_dataset.cache()` decodes every file
once into a ClipBank, `bank.loader(..., augment=True)` then builds each batch on the GPU without touching a
file again, and one mining round adds the negative windows the trained model still fires on (`det_curve` -> `scan_files` ->
`hard_negatives` -> `bank.add_pcm`) before the last epochs.  `--audit` prints what the bank holds (levels, clipping, silent and
overlong clips, duplicates, files shared with the validation list) and `--crop active` draws the window of a
clip longer than `--duration` around its active region instead of uniformly.

    PYTHONPATH=. python examples/train_from_bank.py [--epochs 6] [--mine-after 3] [--data DIR] [--lr 1e-4] [--duration 1.0] [--background DIR]
                                                    [--audit] [--crop active]
"""
import argparse
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.optim as optim  # noqa: E402

from train_from_files import run_epoch, split  # noqa: E402  (the same loop bodies)
from wakeword_jupyterlab_amd import AudioConfig, AudioProcessor, DataLoader, WakewordDataset, WakewordModel  # noqa: E402
from wakeword_jupyterlab_amd.scan import det_curve, scan_files  # noqa: E402
from wakeword_jupyterlab_amd.synth import create_sample_data  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--mine-after", type=int, default=3, help="epochs before the mining round")
    ap.add_argument("--data", default=".")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--duration", type=float, default=AudioConfig.DURATION, help="clip length in seconds, 0.25 .. 1.0")
    ap.add_argument("--background", default=None, help="directory of background noise files (WAV / FLAC) mixed into the training clips")
    ap.add_argument("--fa-per-hour", type=float, default=0.5, help="the operating point the mining threshold is taken from")
    ap.add_argument("--audit", action="store_true", help="print the audit of the training bank, and its overlap with the validation bank")
    ap.add_argument("--crop", default=None, choices=["active"], help="draw the windows of long clips around their active region")
    a = ap.parse_args()
    device = torch.device("cuda")
    wdir, ndir = os.path.join(a.data, "wakeword_data"), os.path.join(a.data, "negative_data")
    if not os.path.exists(wdir) or len(os.listdir(wdir)) == 0:
        create_sample_data(a.data)
    wake = [f for ext in ("*.wav", "*.flac") for f in glob.glob(os.path.join(wdir, ext))]
    neg = [f for ext in ("*.wav", "*.flac") for f in glob.glob(os.path.join(ndir, ext))]
    w_tr, w_va, _ = split(wake)
    n_tr, n_va, _ = split(neg)
    audio_config = type("AudioConfig", (AudioConfig,), {"DURATION": a.duration})
    processor = AudioProcessor(audio_config)
    if a.background:
        processor.set_background_noise(a.background)
    model = WakewordModel(audio_config=audio_config).to(device)
    bank = WakewordDataset(w_tr, n_tr, processor, augment=True).cache()           # every training file decoded once, onto the GPU
    st = bank.stats
    print(f"{bank} -- built at {st['files_per_second']:.0f} files/s, {st['audio_seconds_per_second']:.0f} s of audio/s")
    val_bank = WakewordDataset(w_va, n_va, processor, augment=False).cache()
    if a.audit:
        audit = bank.audit()
        print(audit.report())
        print(f"duplicate groups: {audit.duplicates()}")
        print(f"entries shared with the validation list (train, validation): {audit.duplicates(other=val_bank.audit())}")
    train_loader = bank.loader(a.batch_size, shuffle=True, augment=True, crop=a.crop)
    val_loader = DataLoader(val_bank, batch_size=a.batch_size, shuffle=False)
    criterion = nn.CrossEntropyLoss().to(device)
    optimizer = optim.Adam(model.parameters(), lr=a.lr, weight_decay=1e-5)
    for epoch in range(a.epochs):
        if epoch == a.mine_after:                                                 # one mining round on the training negatives
            model.eval()
            curve = det_curve(model, w_tr, n_tr, hop_samples=160, smooth=3)
            theta = curve.threshold_for(a.fa_per_hour) or 0.5
            pcm, files, times = scan_files(model, n_tr).hard_negatives(theta * 0.8, smooth=3)
            bank.add_pcm(pcm, 0)
            print(f"mined {pcm.shape[0]} windows at theta {theta * 0.8:.3f}: {bank}")
        tl, ta = run_epoch(model, train_loader, criterion, device, optimizer)     # len(train_loader) follows the bank
        vl, va = run_epoch(model, val_loader, criterion, device)
        print(f"Epoch {epoch + 1}/{a.epochs}  Train Loss: {tl:.4f}, Train Acc: {ta:.2f}%  Val Loss: {vl:.4f}, Val Acc: {va:.2f}%")
    torch.save({"model_state_dict": model.state_dict(), "device": str(device)}, os.path.join(a.data, "final_wakeword_model.pth"))


if __name__ == "__main__":
    main()
