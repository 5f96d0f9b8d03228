"""MI355X-native (gfx950 / CDNA4) fusion train / inference path for multimodal emotion recognition.

Drop-in for Wionerlol/MultimodalEmotionRecognition's ``src/models`` API on hand-written HIP
kernels (``csrc/`` -> ``libmer_hip.so``, C-ABI in ``include/mer.h``).
"""
from ._lib import LIB, MerKernelError, available, lib_path  # noqa: F401


def __getattr__(name):
    # reference-named model classes, imported lazily (src/models/{fusion,video,wavlm_audio,audio}.py)
    if name == "FusionModel":
        from .fusion import FusionModel
        return FusionModel
    if name == "VideoNet":
        from .video import VideoNet
        return VideoNet
    if name == "WavLMAudioEncoder":
        from .wavlm_audio import WavLMAudioEncoder
        return WavLMAudioEncoder
    if name in {"AudioNet", "AudioCNN", "AudioResNet18", "SpecAugment"}:
        from . import audio
        return getattr(audio, name)
    # the validation loop and the per-stage epoch driver (src/train.py:247-301, 736-768, 1066-1150; src/eval.py)
    if name in {"evaluate", "fit", "cosine_scheduler", "load_training_state"}:
        from . import train
        return getattr(train, name)
    if name == "FusedAdam":
        from .optim import FusedAdam
        return FusedAdam
    if name == "EvalMetrics":
        from .metrics import EvalMetrics
        return EvalMetrics
    if name == "evaluate_checkpoint":
        from .eval import evaluate_checkpoint
        return evaluate_checkpoint
    # the emotion timeline over a recording (timeline.py, optimized_runtime.py)
    if name in {"plan_windows", "WindowPlan"}:
        from . import timeline
        return getattr(timeline, name)
    if name == "process_recording":
        from .optimized_runtime import process_recording
        return process_recording
    raise AttributeError(name)


__all__ = ["LIB", "MerKernelError", "available", "lib_path", "FusionModel", "VideoNet", "WavLMAudioEncoder",
           "AudioNet", "AudioCNN", "AudioResNet18", "SpecAugment", "evaluate", "fit", "cosine_scheduler", "EvalMetrics", "evaluate_checkpoint",
           "plan_windows", "WindowPlan", "process_recording", "FusedAdam", "load_training_state"]
