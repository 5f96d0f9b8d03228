"""Evaluation metrics accumulated on the device (``src/train.py:262-301``, ``src/utils/metrics.py``).

One ``mer_eval_accum`` launch per batch adds the batch's loss terms and its (label, prediction) counts into a
small state in device memory (``include/mer.h``: ``conf[C*C]``, ``n``, ``invalid``, three fp64 sums); the host
reads it once per evaluation.  Everything after that read is plain host arithmetic (``metrics_from_state``).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

State = Tuple[np.ndarray, int, int, float, float, float]  # conf [C, C] int64, n, invalid, loss/cls/con sums


def macro_f1_from_confusion(conf) -> float:
    """sklearn ``f1_score(average="macro")`` from a confusion matrix (rows = targets, columns = predictions):
    the mean of 2tp / (2tp + fp + fn) over the classes present in predictions or targets (row sum + column sum
    > 0), 0.0 for a class with a zero denominator, 0.0 for an empty matrix.  The only F1 formula in the tree."""
    conf = np.asarray(conf, dtype=np.int64)
    rows, cols, diag = conf.sum(axis=1).tolist(), conf.sum(axis=0).tolist(), np.diagonal(conf).tolist()
    f1s = []
    for tp, r, c in zip(diag, rows, cols):
        if r + c == 0:
            continue
        denom = 2 * tp + (c - tp) + (r - tp)
        f1s.append(0.0 if denom == 0 else 2 * tp / denom)
    return float(sum(f1s) / len(f1s)) if f1s else 0.0


def confusion_from_preds(preds: torch.Tensor, targets: torch.Tensor) -> np.ndarray:
    """Confusion matrix over the sorted distinct values of ``preds`` and ``targets`` (any integers)."""
    preds, targets = preds.reshape(-1).cpu(), targets.reshape(-1).cpu()
    values, inv = torch.unique(torch.cat([preds, targets]), return_inverse=True)
    k = int(values.numel())
    p, t = inv[:preds.numel()], inv[preds.numel():]
    return torch.bincount(t * k + p, minlength=k * k).reshape(k, k).numpy()


def metrics_from_state(state: State) -> dict:
    """{"loss", "cls_loss", "contrastive_loss", "acc", "f1", "confusion", "n"} from a raw state; host code only.

    The three losses are the sums divided by ``n``, the samples actually seen (as ``train_one_epoch`` does).  The
    reference divides by ``len(loader.dataset)`` (train.py:296-298), which is the same number for a loader that
    drops nothing."""
    conf, n, _invalid, loss_sum, cls_sum, con_sum = state
    conf = np.asarray(conf, dtype=np.int64)
    n = int(n)
    d = max(n, 1)
    return {"loss": float(loss_sum) / d, "cls_loss": float(cls_sum) / d, "contrastive_loss": float(con_sum) / d,
            "acc": int(np.trace(conf)) / n if n else 0.0, "f1": macro_f1_from_confusion(conf) if n else 0.0,
            "confusion": conf, "n": n}


def merge_states(state: State, group=None) -> State:
    """Sum the raw state across ranks, so every rank computes the same global metrics: a host-side all-reduce on
    ``dist.cpu_group()`` (or the given gloo group), int64 for the counters and float64 for the sums.  A no-op for
    a single process."""
    from . import dist as D

    if not D.is_dist():
        return state
    import torch.distributed as td

    conf, n, invalid, loss_sum, cls_sum, con_sum = state
    conf = np.asarray(conf, dtype=np.int64)
    group = group if group is not None else D.cpu_group()
    counts = torch.from_numpy(np.concatenate([conf.reshape(-1), np.array([n, invalid], dtype=np.int64)]))
    sums = torch.tensor([loss_sum, cls_sum, con_sum], dtype=torch.float64)
    td.all_reduce(counts, op=td.ReduceOp.SUM, group=group)
    td.all_reduce(sums, op=td.ReduceOp.SUM, group=group)
    counts = counts.numpy()
    return (counts[:-2].reshape(conf.shape).copy(), int(counts[-2]), int(counts[-1]), float(sums[0]), float(sums[1]),
            float(sums[2]))


class EvalMetrics:
    """Running evaluation totals in device memory (train.py:257-301 without its three ``.item()`` syncs per batch).

    ``update`` is one kernel launch and no host sync; ``state`` is the one device-to-host copy."""

    def __init__(self, num_classes: int, device, label_smoothing: float = 0.0, late: bool = False,
                 align_weight: float = 0.0):
        from . import kernels as K

        self.num_classes = int(num_classes)
        if self.num_classes < 1:
            raise ValueError("num_classes must be >= 1")
        self.label_smoothing, self.late, self.align_weight = float(label_smoothing), bool(late), float(align_weight)
        self._state = torch.zeros(K.eval_state_words(self.num_classes), dtype=torch.int64, device=device)

    def reset(self) -> None:
        self._state.zero_()

    def update(self, outputs: torch.Tensor, labels: torch.Tensor,
               align_loss: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Add one batch (logits, or probabilities when ``late``); returns its top-1 predictions (device int64)."""
        from . import kernels as K

        outputs = outputs.detach().contiguous().float()
        if outputs.dim() != 2 or outputs.shape[1] != self.num_classes:
            raise ValueError(f"outputs must be [B, {self.num_classes}]")
        preds = torch.empty(outputs.shape[0], device=outputs.device, dtype=torch.int64)
        if align_loss is not None:
            align_loss = align_loss.detach().contiguous().float()
        K.eval_accum(outputs, labels.contiguous(), self._state, self.label_smoothing, self.late,
                     align_loss=align_loss, align_weight=self.align_weight, preds=preds)
        return preds

    def state(self) -> State:
        c = self.num_classes
        host = self._state.cpu().numpy()
        sums = host[c * c + 2:].view(np.float64)
        return (host[:c * c].reshape(c, c).copy(), int(host[c * c]), int(host[c * c + 1]), float(sums[0]),
                float(sums[1]), float(sums[2]))

    def compute(self) -> dict:
        state = self.state()
        if state[2] > 0:
            raise ValueError(f"{state[2]} labels outside [0, {self.num_classes}) were seen during the evaluation")
        return metrics_from_state(state)
