"""The callers the drop-in serves: the batched eval loop and single-file predict.

  evaluate(model, loader, device)   <- notebook cell 17 lines 8-19 (wakeword_training.ipynb:727+) and
                                       WakewordTrainer.validate (wakeword_training_script.py:269-289)
  predict_wakeword(path, model, processor, device, threshold=0.8)
                                    <- notebook cell 19 (wakeword_training.ipynb:871-893)
  evaluate_pcm(model, pcm, batch)   the same loop fed with PCM already in HBM (bench / multi-GPU path)
  evaluate_report(model, loader)    cell 17's loop with its counters kept on the device: one launch per batch, one copy at the end,
                                    a metrics.ClipReport (confusion, sklearn's report, ROC, AUC, EER, operating points) as the result
  evaluate_report_pcm(model, pcm, batch, labels)   the same from PCM and labels already in HBM
"""
from __future__ import annotations

import numpy as np
import torch


def evaluate(model, loader, device, criterion=None):
    """Returns (all_preds, all_labels[, mean loss, accuracy %]).  `loader` yields (data [B,1,80,T], target [B,1])."""
    model.eval()
    all_preds, all_labels = [], []
    total_loss, correct, total, n_batches = 0.0, 0, 0, 0
    with torch.no_grad():
        for data, target in loader:
            data, target = data.to(device), target.to(device).squeeze()
            output = model(data)
            if criterion is not None:
                total_loss += criterion(output, target.reshape(-1)).item()
            _, predicted = torch.max(output, 1)
            total += target.numel()
            correct += (predicted == target.reshape(-1)).sum().item()
            n_batches += 1
            all_preds.extend(predicted.cpu().numpy())
            all_labels.extend(np.atleast_1d(target.cpu().numpy()))
    if criterion is None:
        return all_preds, all_labels
    return all_preds, all_labels, total_loss / max(1, n_batches), 100.0 * correct / max(1, total)


def predict_wakeword(audio_file_path, model, processor, device, threshold=0.8):
    """Single file -> (is_wakeword, probability); (False, 0.0) when the file cannot be processed."""
    model.eval()
    mel_spec = processor.process_audio_file(audio_file_path, augment=False)
    if mel_spec is None:
        print(f"Error processing audio file: {audio_file_path}")
        return False, 0.0
    mel_tensor = torch.FloatTensor(np.asarray(mel_spec, dtype=np.float32)).unsqueeze(0).unsqueeze(0).to(device)
    with torch.no_grad():
        output = model(mel_tensor)
        probabilities = torch.softmax(output, dim=1)
        wakeword_prob = probabilities[0][1].item()
    return wakeword_prob >= threshold, wakeword_prob


def evaluate_pcm(model, pcm: torch.Tensor, batch_size: int = 4096, normalize: bool = True):
    """PCM [N, n<=16000] on the device (n <= the model's clip length for a model built with another DURATION) -> (logits [N,2], predictions [N])
    in batches of `batch_size`."""
    model.eval()
    outs = []
    with torch.no_grad():
        for s in range(0, pcm.shape[0], batch_size):
            outs.append(model.forward_pcm(pcm[s:s + batch_size], normalize))
    logits = torch.cat(outs) if outs else torch.empty((0, 2), device=pcm.device)
    return logits, (torch.max(logits, 1)[1] if len(logits) else torch.empty(0, dtype=torch.long, device=pcm.device))


def _report_labels(target, n: int, device) -> torch.Tensor:
    if not isinstance(target, torch.Tensor):
        target = torch.as_tensor(target)
    if target.dtype.is_floating_point or target.dtype == torch.bool:
        raise TypeError(f"labels: expected integer class labels, got {target.dtype}")
    target = target.to(device=device, dtype=torch.int64).reshape(-1)
    if target.shape[0] != n:
        raise ValueError(f"labels: expected {n} labels for {n} clips, got {target.shape[0]}")
    return target


def evaluate_report(model, loader, device=None, thresholds=(0.8,), ledger=None):
    """Notebook cell 17's loop without its per-batch copies: every batch's logits and labels go into a ww_clip_metrics record on the
    device (one launch, in stream order) and the record is read once, after the last batch.  Returns a metrics.ClipReport: `.confusion`,
    `.classification_report()`, `.summary()` are cell 17's numbers; `.at(p)` for each p of `thresholds`, `.roc()`, `.auc`, `.eer` and
    `.threshold_for(max_fpr)` answer the deployment question.  `loader` yields (data [B,1,80,T], target [B,1] or [B]).  `ledger` (a
    ledger.ClipLedger): the same pass also scatters every row into it by the loader's `last_entries` (bank.loader, dataset.loader), under
    the ledger's current epoch -- on a fresh ledger no epoch bit is set, and `ledger.read().misclassified()` names the clips behind the
    confusion matrix."""
    from . import ops
    model.eval()
    device = torch.device(device) if device is not None else next(model.parameters()).device
    state = ops.new_clip_metrics(device, thresholds)
    with torch.no_grad():
        for data, target in loader:
            output = model(data.to(device))
            labels = _report_labels(target, output.shape[0], device)
            ops.clip_metrics_update(output, labels, state)
            if ledger is not None:
                entries = getattr(loader, "last_entries", None)
                if entries is None:
                    raise TypeError(f"evaluate_report(ledger=): {type(loader).__name__} has no `last_entries` to name its rows by")
                ledger.update(entries, output, labels)
    return ops.read_clip_metrics(state)


def evaluate_report_pcm(model, pcm: torch.Tensor, batch_size: int = 4096, labels=None, thresholds=(0.8,), normalize: bool = True):
    """`evaluate_report` for PCM [N, n<=16000] and labels [N] already on the device, in batches of `batch_size`."""
    from . import ops
    if labels is None:
        raise TypeError("evaluate_report_pcm: labels [N] are required (a report needs the truth)")
    model.eval()
    labels = _report_labels(labels, pcm.shape[0], pcm.device)
    state = ops.new_clip_metrics(pcm.device, thresholds)
    with torch.no_grad():
        for s in range(0, pcm.shape[0], batch_size):
            ops.clip_metrics_update(model.forward_pcm(pcm[s:s + batch_size], normalize), labels[s:s + batch_size], state)
    return ops.read_clip_metrics(state)
