"""Batch-inference runtime mirroring ``src/optimized_runtime.py`` (TorchModelRunner) and the tensor path
of ``src/inference_worker.py:_process_batch`` (stack -> predict_probs -> per-row top-1).

Checkpoints use the reference's format ``{"model": state_dict, "val_f1", "config"}`` and its state-dict
key names, so a checkpoint written by the reference's train.py loads unchanged.  Loading is
``torch.load(weights_only=True)`` (tensors + plain containers only).
"""
from __future__ import annotations

from pathlib import Path
from typing import Any, Dict, List, Optional

import torch
from .train import build_model

FOUR_CLASS_LABELS = ["neutral_calm", "happy", "negative", "surprised"]
EIGHT_CLASS_LABELS = ["neutral", "calm", "happy", "sad", "angry", "fearful", "disgust", "surprised"]
FUSION_MODES = {"audio", "video", "late", "concat", "gated", "xattn", "xattn_concat", "xattn_gated"}
SAMPLE_RATE = 16000  # the reference's audio rate (ravdess.py:505, WavLM and the mel front end alike)


def labels_for_num_classes(num_classes: int) -> List[str]:
    return EIGHT_CLASS_LABELS if num_classes == 8 else FOUR_CLASS_LABELS


# (state-dict prefix that must be present, fusion mode, xattn head) in the precedence order of
# optimized_runtime.py:22-37; fusion checkpoints carry both encoders, single-encoder ones one of them.
_FUSION_SIGNATURES = (("xattn_gate.", "xattn", "gated"), ("xattn_mlp.", "xattn", "concat"),
                      ("fusion.", "concat", "concat"), ("gate.", "gated", "gated"))
_SINGLE_SIGNATURES = ((("encoder.", "wavlm."), "audio"), (("backbone.",), "video"))
# config key -> build_model keyword default (the runner reads these from checkpoint["config"])
_CONFIG_DEFAULTS = dict(
    xattn_d_model=128, xattn_heads=4, xattn_attn_dropout=0.1, xattn_stochastic_depth=0.1,
    xattn_use_emotion_prior=False, xattn_emotion_prior_dim=8, xattn_emotion_prior_hidden_dim=64,
    xattn_emotion_prior_dropout=0.1, temporal_pooling="mean", temporal_num_heads=4, temporal_num_layers=1,
    temporal_dropout=0.1, audio_n_mels=64, use_resnet_audio=True, fusion_align_mode="none", fusion_align_dim=256,
    fusion_align_temperature=0.07)


def _has_prefix(keys, *prefixes) -> bool:
    return any(k.startswith(prefixes) for k in keys)


def infer_model_signature(state_dict: Dict[str, torch.Tensor]):
    """(fusion mode, xattn head) from the checkpoint's key prefixes -- optimized_runtime.py:22-37."""
    keys = list(state_dict)
    if _has_prefix(keys, "audio_model.") and _has_prefix(keys, "video_model."):
        for prefix, mode, head in _FUSION_SIGNATURES:
            if _has_prefix(keys, prefix):
                return mode, head
        return "late", "concat"
    for prefixes, mode in _SINGLE_SIGNATURES:
        if _has_prefix(keys, *prefixes):
            return mode, "concat"
    raise RuntimeError("Unable to infer model type from checkpoint state_dict keys.")


def checkpoint_uses_wavlm(state_dict: Dict[str, torch.Tensor]) -> bool:
    """optimized_runtime.py:40-41."""
    return _has_prefix(list(state_dict), "audio_model.wavlm.", "wavlm.")


def checkpoint_uses_resnet_audio(state_dict: Dict[str, torch.Tensor]):
    """Which mel encoder a checkpoint without "config" holds, from its keys: ``encoder.conv1.`` is AudioResNet18,
    ``encoder.features.`` is AudioCNN (with or without the ``audio_model.`` prefix); None when it holds neither."""
    keys = list(state_dict)
    if _has_prefix(keys, "audio_model.encoder.conv1.", "encoder.conv1."):
        return True
    if _has_prefix(keys, "audio_model.encoder.features.", "encoder.features."):
        return False
    return None


class TorchModelRunner:
    """optimized_runtime.py:44-108 on the MI355X kernels.

    ``enable_dynamic_quant`` selects the INT8 linear path (per-tensor symmetric int8 weights, dynamic
    per-row int8 activations, int32 MFMA accumulation) that mirrors ``quantize_dynamic({nn.Linear})``;
    in the reference it is CPU-only (optimized_runtime.py:95-96), here it runs on the GPU.

    Mel checkpoints (``AudioNet``, the reference's default audio model): ``predict_probs`` takes
    the log-mel batch ``[B, 1, n_mels, T]`` or a waveform batch ``[B, 1, S]``, which it passes through
    ``clips.log_mel`` first, so the same loader batches serve both kinds of checkpoint.
    """

    def __init__(self, checkpoint_path: Optional[str] = None, device: str = "cuda", fallback_fusion: str = "xattn",
                 enable_dynamic_quant: bool = False, checkpoint: Optional[Dict[str, Any]] = None):
        self.device = torch.device(device)
        if checkpoint is None:
            checkpoint = torch.load(Path(checkpoint_path).expanduser(), map_location="cpu", weights_only=True)
        if not isinstance(checkpoint, dict) or "model" not in checkpoint:
            raise RuntimeError("Checkpoint format not supported. Expected {'model': state_dict, 'config': ...}.")
        self.config = checkpoint.get("config", {}) or {}
        state_dict = checkpoint["model"]
        if "fusion" in self.config:
            self.fusion_mode = str(self.config.get("fusion", fallback_fusion))
            xattn_head = str(self.config.get("xattn_head", "concat"))
        else:
            self.fusion_mode, xattn_head = infer_model_signature(state_dict)
        if self.fusion_mode not in FUSION_MODES:
            raise ValueError(f"Unsupported fusion mode: {self.fusion_mode}")
        self.num_classes = int(self.config.get("num_classes", 8))
        self.use_wavlm = bool(self.config.get("use_wavlm", checkpoint_uses_wavlm(state_dict)))
        self.labels = labels_for_num_classes(self.num_classes)
        kw = {k: self.config.get(k, d) for k, d in _CONFIG_DEFAULTS.items()}
        self.uses_mel = not self.use_wavlm and self.fusion_mode != "video"
        if self.uses_mel:
            if "use_resnet_audio" not in self.config:
                from_keys = checkpoint_uses_resnet_audio(state_dict)
                if from_keys is not None:
                    kw["use_resnet_audio"] = from_keys
            if enable_dynamic_quant:
                raise NotImplementedError("enable_dynamic_quant with a mel (AudioNet) checkpoint is not built: INT8 "
                                          "covers the WavLM models")
        self.n_mels = int(kw["audio_n_mels"])
        model = build_model(num_classes=self.num_classes, fusion=self.fusion_mode, pretrained_video=False,
                            xattn_head=xattn_head, use_wavlm=self.use_wavlm, **kw)
        missing, unexpected = model.load_state_dict(state_dict, strict=False)
        if unexpected:
            raise RuntimeError(f"Unexpected checkpoint keys ({len(unexpected)}): {unexpected[:8]}")
        if len(missing) > 32:
            raise RuntimeError(f"Too many missing keys when loading checkpoint ({len(missing)}). "
                               "Checkpoint architecture does not match the inferred runtime model.")
        self.model = model.to(self.device).eval()
        self.int8 = bool(enable_dynamic_quant)
        if self.int8:
            from .int8 import quantize_dynamic_hip
            quantize_dynamic_hip(self.model)

    def predict_probs(self, videos: torch.Tensor, audios: torch.Tensor) -> torch.Tensor:
        """optimized_runtime.py:99-108: softmax probabilities (late mode already returns probabilities)."""
        with torch.inference_mode():
            videos = videos.to(self.device, non_blocking=True)
            audios = audios.to(self.device, non_blocking=True)
            if self.uses_mel and audios.dim() == 3:  # a waveform batch [B, 1, S] for a mel checkpoint
                from .clips import log_mel
                audios = log_mel(audios, n_mels=self.n_mels)
            if self.fusion_mode == "audio":
                outputs = self.model(audios)
            elif self.fusion_mode == "video":
                outputs = self.model(videos)
            else:
                outputs = self.model(videos, audios)
            probs = outputs if self.fusion_mode == "late" else _softmax(outputs)
        return probs.detach().cpu()

    def predict_timeline(self, frames_u8: Optional[torch.Tensor], waveform: Optional[torch.Tensor], fps, *,
                         window_sec: float = 3.0, hop_sec: float = 1.0, frames_per_window: int = 8,
                         frame_grid: str = "window", include_tail: bool = False, smooth_radius: int = 0,
                         max_windows_per_batch: int = 64, sample_rate: int = SAMPLE_RATE, face_boxes=None,
                         pad_ratio: float = 0.3, debug: bool = False) -> Dict[str, Any]:
        """One prediction per window over a whole decoded recording, every frame encoded once.

        ``frames_u8`` ``[N, H, W, 3]`` uint8 RGB at ``fps`` and the mono 16 kHz ``waveform`` (fp32, any shape), host
        or device.  ``timeline.plan_windows`` fixes the windows; the recording crosses PCIe once; the frame trunk runs
        on the plan's UNIQUE frames only (in eval mode it is a per-frame function), their features are gathered to the
        windows' slots, the audio windows are offsets into the one waveform, and ``forward_from_frame_features`` runs
        on at most ``max_windows_per_batch`` windows at a time.  With ``frame_grid="window"`` each row is what
        ``predict_probs`` gives for that window cut out by hand (same network, other batch shapes);
        ``frame_grid="shared"`` samples one grid for the whole recording so that overlapping windows share frames.

        ``audio`` mode skips the frame work (``frames_u8`` may be None); ``video`` mode uses the video path only (the
        waveform then only fixes the recording's length in samples, and may be None: ``round(N / fps * 16000)``).

        Returns ``probs`` / ``smoothed`` ``[Nw, C]`` (``smoothed``: the centred moving average over ``2 *
        smooth_radius + 1`` windows, clipped to the recording), ``top1`` ``[Nw]`` int32 (argmax of ``smoothed``),
        ``starts_sec``, ``window_seconds``, ``labels``, ``num_windows``, ``num_unique_frames`` and ``num_frame_slots``
        (``Nw * T``).

        ``sample_rate``: the waveform's rate.  Any rate other than 16000 resamples the whole recording once on the
        device (``clips.resample_clips``, scipy ``resample_poly``'s filter) before the windows are planned; the result
        is ``predict_timeline`` of that resampled waveform.  At 16000 nothing changes.

        ``face_boxes``: the face crop of the reference's ``use_face_crop`` (``crop_with_padding``, each side padded
        by ``pad_ratio``), for a checkpoint trained on face crops.  ``None``: whole frames, the bits this method
        always gave.  One raw detector box ``(x1, y1, x2, y2)``: every frame is cropped to it.  An integer array
        ``[N, 4]``: one box per decoded frame, an empty row meaning "no detection" (the whole frame is used).  Only
        the rectangles of the unique sampled frames are computed (``clips.crop_rects``); each such frame is cropped
        with its OWN box on the device (``clips.gather_preprocess_frames(..., rects=...)``) and still encoded once.
        This DEPARTS from the reference, which detects once per window and reuses that box for the window's frames
        (preprocess.py ``load_video_frames``): here a box belongs to a frame, because frames are shared between
        windows.  With one box for the recording, or boxes constant over a window, the two coincide.  Face
        detection itself is the caller's.  A ``face_boxes`` of another shape or dtype, or boxes given to an
        audio-only checkpoint, raise ``ValueError`` before any device work.

        ``debug=True`` adds ``debug``: the preprocessed unique frames ``[U, 3, 112, 112]`` (device), ``unique_idx``,
        ``inverse``, the ``rects`` used (or None) and ``trunk_batches``, the frame count of every trunk call."""
        from . import clips
        from . import kernels as K
        from .timeline import checked_face_boxes, plan_windows

        if face_boxes is not None:
            if self.fusion_mode == "audio":
                raise ValueError("face_boxes given to an audio-only checkpoint: it reads no frames")
            if frames_u8 is None or frames_u8.dim() != 4:
                raise ValueError("frames_u8 must be uint8 [N, H, W, 3] (RGB)")
            boxes = checked_face_boxes(face_boxes, int(frames_u8.shape[0]))
        if int(sample_rate) != SAMPLE_RATE:
            clips.resample_ratio(sample_rate, SAMPLE_RATE)  # refuses a non-positive rate before any device work
        if self.device.type != "cuda":
            raise RuntimeError("predict_timeline runs on the MI355X kernels; build the runner on a GPU device "
                               "(device='cuda')")
        chunk_w, radius = int(max_windows_per_batch), int(smooth_radius)
        if chunk_w < 1:
            raise ValueError(f"max_windows_per_batch must be at least 1, got {max_windows_per_batch}")
        if radius < 0:
            raise ValueError(f"smooth_radius must be >= 0, got {smooth_radius}")
        use_video, use_audio = self.fusion_mode != "audio", self.fusion_mode != "video"
        if use_video:
            if frames_u8 is None or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
                raise ValueError("frames_u8 must be uint8 [N, H, W, 3] (RGB)")
            n_frames = int(frames_u8.shape[0])
        else:
            n_frames = int(frames_u8.shape[0]) if frames_u8 is not None else 1
        if waveform is None:
            if use_audio:
                raise ValueError(f"{self.fusion_mode} mode needs the recording's waveform")
            if not float(fps) > 0:
                raise ValueError(f"fps must be positive, got {fps!r}")
            n_samples = int(round(n_frames / float(fps) * SAMPLE_RATE))
        else:
            if waveform.dtype != torch.float32:
                raise ValueError("waveform must be fp32")
            if int(sample_rate) != SAMPLE_RATE:
                waveform = clips.resample_clips(waveform.reshape(-1), int(sample_rate), SAMPLE_RATE,
                                                device=self.device).reshape(-1)
            n_samples = int(waveform.numel())
        plan = plan_windows(n_frames, fps, n_samples, SAMPLE_RATE, window_sec, hop_sec,
                            frames_per_window if use_video else 1, frame_grid, include_tail)
        Nw, T = plan.num_windows, plan.frames_per_window
        U = int(plan.unique_idx.numel()) if use_video else 0
        with torch.inference_mode():
            v_feat = audio = x = rects = None
            trunk_batches = []
            if use_video:
                frames = frames_u8 if frames_u8.is_cuda else clips._h2d(frames_u8.contiguous(), self.device)
                if face_boxes is not None:  # the unique frames' own boxes -> their rectangles, host arithmetic
                    own = boxes[plan.unique_idx.long().numpy()] if boxes.shape[0] == n_frames else \
                        boxes.repeat(U, axis=0)
                    rects = clips.crop_rects(frames.shape[1], frames.shape[2], own, pad_ratio)
                x = clips.gather_preprocess_frames(frames, plan.unique_idx, rects=rects)
                vnet = self.model if self.fusion_mode == "video" else self.model.video_model
                step = chunk_w * T
                feats = [vnet.backbone(x[i:i + step]).reshape(-1, vnet.embedding_dim) for i in range(0, U, step)]
                trunk_batches = [min(step, U - i) for i in range(0, U, step)]
                feats = feats[0] if len(feats) == 1 else torch.cat(feats)
                v_feat = K.rows_gather(feats, plan.inverse.reshape(-1)).view(Nw, T, vnet.embedding_dim)
            if use_audio:
                audio = clips.waveform_windows(waveform, plan.starts, plan.lengths, plan.target, device=self.device)
                if self.uses_mel:
                    audio = clips.log_mel(audio, n_mels=self.n_mels)
            rows = []
            for i in range(0, Nw, chunk_w):
                if self.fusion_mode == "audio":
                    out = self.model(audio[i:i + chunk_w])
                elif self.fusion_mode == "video":
                    out = self.model.forward_from_frame_features(v_feat[i:i + chunk_w])
                else:
                    out = self.model.forward_from_frame_features(v_feat[i:i + chunk_w], audio[i:i + chunk_w])
                rows.append(out.contiguous().float() if self.fusion_mode == "late" else _softmax(out))
            probs = rows[0] if len(rows) == 1 else torch.cat(rows)
            smoothed, top1 = K.timeline_smooth(probs, radius)
            # one device-to-host copy: the class indices ride along as exactly representable floats
            host = torch.cat([probs, smoothed, top1.to(torch.float32)[:, None]], dim=1).cpu()
        C = probs.shape[1]
        res = {"probs": host[:, :C].contiguous(), "smoothed": host[:, C:2 * C].contiguous(),
               "top1": host[:, 2 * C].to(torch.int32), "starts_sec": list(plan.starts_sec), "labels": self.labels,
               "num_windows": Nw, "num_unique_frames": U, "num_frame_slots": Nw * T if use_video else 0,
               "window_seconds": float(window_sec)}
        if debug:
            res["debug"] = dict(frames=x, unique_idx=plan.unique_idx, inverse=plan.inverse, rects=rects,
                                trunk_batches=trunk_batches)
        return res


    def open_stream_pool(self, max_sessions: int = 16, **kw):
        """A ``streaming.StreamingSessionPool`` on this runner: live sessions whose audio, frames and frame features
        stay in device rings, every sample resampled once, every frame encoded at most once, all due sessions
        predicted in one batch.  GPU runners only (``RuntimeError`` otherwise)."""
        from .streaming import StreamingSessionPool

        return StreamingSessionPool(self, max_sessions, **kw)


def _softmax(x: torch.Tensor) -> torch.Tensor:
    from . import kernels as K

    x = x.contiguous().float()
    out = torch.empty_like(x)
    pa = torch.empty_like(x)
    K.softmax_avg_fwd(x, x, out, pa, torch.empty_like(x))  # (softmax + softmax) / 2 == softmax
    return out


def process_batch(runner: TorchModelRunner, videos: List[torch.Tensor], audios: List[torch.Tensor]):
    """Tensor path of inference_worker.py:_process_batch (131-147): stack, predict, per-row top-1."""
    v = torch.stack(videos, dim=0)
    a = torch.stack(audios, dim=0)
    probs = runner.predict_probs(v, a)
    return [_result_row(runner, row) for row in probs]


def _result_row(runner: TorchModelRunner, row: torch.Tensor, top: Optional[int] = None) -> Dict[str, Any]:
    """One clip's result in the worker's format (inference_worker.py:139-147); ``top``: a top-1 already known."""
    top = int(row.argmax().item()) if top is None else int(top)
    return {"labels": runner.labels, "probs": [round(float(p), 6) for p in row.tolist()],
            "top1": {"label": runner.labels[top], "prob": round(float(row[top].item()), 6)}}


def process_recording(runner: TorchModelRunner, frames_u8: Optional[torch.Tensor], waveform: Optional[torch.Tensor],
                      fps, *, sample_rate: int = SAMPLE_RATE, **kw) -> List[Dict[str, Any]]:
    """``process_batch`` over a whole recording: ``runner.predict_timeline(frames_u8, waveform, fps, **kw)`` as one
    dict per window in ``process_batch``'s format, plus the window's ``start_sec`` and ``window_seconds`` (the keys
    of the streaming session's result, streaming.py:103-115).  With ``smooth_radius > 0`` each dict also carries
    ``smoothed``: the smoothed row in the same format, its top-1 the device's (lowest index on ties).
    ``sample_rate``: the waveform's rate; any rate other than 16000 is resampled once on the device.  ``face_boxes`` /
    ``pad_ratio`` (in ``kw``) crop every frame to its face box first, as ``predict_timeline`` documents."""
    if int(sample_rate) != SAMPLE_RATE:
        kw["sample_rate"] = int(sample_rate)
    res = runner.predict_timeline(frames_u8, waveform, fps, **kw)
    out = []
    for w, row in enumerate(res["probs"]):
        d = _result_row(runner, row)
        d["start_sec"], d["window_seconds"] = res["starts_sec"][w], res["window_seconds"]
        if int(kw.get("smooth_radius", 0)) > 0:
            d["smoothed"] = _result_row(runner, res["smoothed"][w], top=int(res["top1"][w]))
        out.append(d)
    return out
