"""Test-set entry point mirroring ``src/eval.py`` (41-63, 218-275): load a checkpoint, run the validation loop
over a loader, print accuracy and macro-F1."""
from __future__ import annotations

from typing import Optional

from .optimized_runtime import TorchModelRunner
from .train import evaluate, make_loss


def evaluate_checkpoint(checkpoint_path, loader, device="cuda", fusion: Optional[str] = None,
                        label_smoothing: float = 0.0) -> dict:
    """eval.py:218-275 for a checkpoint in the reference's format (``train.save_checkpoint`` writes it).

    The model is rebuilt and loaded by ``TorchModelRunner`` (the config keys of eval.py:248-272, the fusion mode
    from the checkpoint's config or its key prefixes); ``fusion`` is the fallback mode when the checkpoint names
    none (eval.py's ``--fusion``).  Runs ``train.evaluate`` -- so, beyond eval.py:41-63, the dict also carries the
    loss and the confusion matrix -- and prints the two lines of eval.py:62-63."""
    runner = TorchModelRunner(str(checkpoint_path), device=device, fallback_fusion=fusion or "xattn")
    mode = runner.fusion_mode
    metrics = evaluate(runner.model, loader, runner.device, make_loss(mode, label_smoothing), mode)
    print(f"Accuracy: {metrics['acc']:.4f}")
    print(f"Macro-F1: {metrics['f1']:.4f}")
    return metrics
