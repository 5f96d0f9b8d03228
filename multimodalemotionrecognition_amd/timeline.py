"""Window plan of an emotion timeline: which samples and which frames each prediction of a long recording reads.

The reference predicts over a stream by rebuilding the last ``window_seconds`` from host buffers at every tick and
running the whole model on it (``backend/app/streaming.py``: ``StreamingEmotionSession.build_window`` / ``infer``).
Over a recording that is already decoded the windows are known up front, so the plan is made once on the host (pure
Python, no device) and ``TorchModelRunner.predict_timeline`` assembles every window on the device from the one
recording: frames through ``clips.gather_preprocess_frames`` on the plan's UNIQUE frame indices, audio through
``clips.waveform_windows`` (offsets into the one waveform).

Rules (all positions are exact rational arithmetic on ``fps``, so a boundary never depends on float rounding):

* ``target = int(sample_rate * window_sec)`` samples per window; window ``w`` starts at sample
  ``s_w = round(w * hop_sec * sample_rate)`` for every ``w`` with ``s_w + target <= n_samples``.  A recording shorter
  than one window gives one window at 0, zero-padded at the end as ``pad_crop_waveforms`` pads a short clip.
  ``include_tail`` adds a last window at ``n_samples - target`` when that start is not there yet: the streaming
  session's "last ``window_seconds``" window.
* window ``w`` covers frames ``[f_w, f_w + n_w)``, ``f_w = floor(s_w / sample_rate * fps)`` (at most the last frame),
  ``n_w = min(n_frames - f_w, ceil(window_sec * fps))``, at least 1.
* ``frame_grid="window"`` (default, the reference's rule, ravdess.py:272-277): ``T`` frames spread evenly over the
  window's own frames, ``f_w + round(linspace(0, n_w - 1, T))``; a window of fewer than ``T`` frames takes each once
  and repeats its last.
* ``frame_grid="shared"`` DEPARTS from the reference's per-window sampling: every window samples the one grid of the
  recording, frame numbers that are multiples of ``q = max(1, ceil(window_sec * fps) // T)``, so that overlapping
  windows pick identical frames and the frame trunk encodes each once: ``index(w, j) = min(n_frames - 1,
  (f_w // q + j) * q)``.  A window then spans ``(T - 1) * q + 1`` frames from the grid point at or before ``f_w``,
  not exactly its own first to last frame.
* face boxes (``predict_timeline(face_boxes=...)``, ``checked_face_boxes``): a box belongs to a FRAME, not to a window
  as in the reference (which detects once per window and reuses that box for its frames), because a frame is shared
  between windows and encoded once.  One box for the recording, or boxes constant over a window: the two coincide.
"""
from __future__ import annotations

import dataclasses
import math
from fractions import Fraction
from typing import List

import numpy as np
import torch

FRAME_GRIDS = ("window", "shared")


@dataclasses.dataclass
class WindowPlan:
    frame_idx: torch.Tensor  # [Nw, T] int32: the recording's frame each slot shows
    unique_idx: torch.Tensor  # [U] int32: sorted unique values of frame_idx (the frames the trunk encodes)
    inverse: torch.Tensor  # [Nw, T] int32: unique_idx[inverse] == frame_idx
    starts: torch.Tensor  # [Nw] int64: first sample of each window
    lengths: torch.Tensor  # [Nw] int64: samples the recording has for it, min(target, n_samples - start)
    starts_sec: List[float]
    target: int  # samples per window
    window_sec: float
    frame_grid: str

    @property
    def num_windows(self) -> int:
        return int(self.starts.numel())

    @property
    def frames_per_window(self) -> int:
        return int(self.frame_idx.shape[1])


def _even_indices(total: int, num: int) -> List[int]:
    """``num`` positions spread evenly over ``range(total)``, first and last included, rounded half to even; fewer
    than ``num`` frames: each once, then the last one again."""
    if total >= num:
        return [int(v) for v in np.linspace(0, total - 1, num=num).round()]
    return [min(j, total - 1) for j in range(num)]


def _rational(x, name: str) -> Fraction:
    try:
        v = Fraction(x) if isinstance(x, (int, Fraction)) else Fraction(float(x)).limit_denominator(1_000_000)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{name} must be a positive finite number, got {x!r}") from None
    if v <= 0:
        raise ValueError(f"{name} must be positive, got {x!r}")
    return v


def window_starts(n_samples: int, sample_rate: int, window_sec, hop_sec, include_tail: bool = False):
    """(starts in samples, target) by the rules in the module docstring."""
    n_samples, sample_rate = int(n_samples), int(sample_rate)
    if n_samples <= 0:
        raise ValueError("empty recording: no audio samples")
    if sample_rate <= 0:
        raise ValueError(f"sample_rate must be positive, got {sample_rate}")
    win, hop = _rational(window_sec, "window_sec"), _rational(hop_sec, "hop_sec")
    target = int(sample_rate * win)
    if target < 1:
        raise ValueError(f"window_sec {window_sec} is shorter than one sample")
    starts, w = [], 0
    while True:
        s = round(w * hop * sample_rate)
        if s + target > n_samples or (starts and s <= starts[-1]):  # (a hop below one sample does not advance)
            break
        starts.append(s)
        w += 1
    if not starts:
        starts = [0]
    elif include_tail and n_samples - target not in starts:
        starts.append(n_samples - target)
    return starts, target


def checked_face_boxes(face_boxes, n_frames: int):
    """``predict_timeline``'s ``face_boxes`` as a host int64 array: ``None`` stays ``None``, one box ``(x1, y1, x2,
    y2)`` for the whole recording gives ``[1, 4]``, a table with one raw detector box per decoded frame gives
    ``[n_frames, 4]`` (an empty row, ``x2 <= x1`` or ``y2 <= y1``: no detection in that frame).  Anything else -- a
    floating-point array, another shape, a table for another number of frames -- is a ``ValueError``.  Host only."""
    if face_boxes is None:
        return None
    a = face_boxes.detach().cpu().numpy() if isinstance(face_boxes, torch.Tensor) else face_boxes
    try:
        a = np.asarray(a)
    except (TypeError, ValueError):
        a = None
    if a is None or a.dtype.kind not in "iu" or a.shape not in ((4,), (int(n_frames), 4)):
        raise ValueError(f"face_boxes must be one integer box (x1, y1, x2, y2) or an integer array [{int(n_frames)}, 4]"
                         f" with one box per decoded frame, got {getattr(a, 'dtype', type(face_boxes))} "
                         f"{getattr(a, 'shape', '')}")
    if a.size and int(np.abs(a.astype(np.int64)).max()) >= 2 ** 30:
        raise ValueError("face_boxes coordinates must be below 2^30")
    return a.astype(np.int64).reshape(-1, 4)


def plan_windows(n_frames: int, fps, n_samples: int, sample_rate: int = 16000, window_sec=3.0, hop_sec=1.0,
                 frames_per_window: int = 8, frame_grid: str = "window", include_tail: bool = False) -> WindowPlan:
    """The windows of a recording of ``n_frames`` frames at ``fps`` and ``n_samples`` samples at ``sample_rate``."""
    if frame_grid not in FRAME_GRIDS:
        raise ValueError(f"unknown frame_grid {frame_grid!r}: one of {FRAME_GRIDS}")
    T, n_frames = int(frames_per_window), int(n_frames)
    if T < 1:
        raise ValueError(f"frames_per_window must be at least 1, got {frames_per_window}")
    if n_frames <= 0:
        raise ValueError("empty recording: no frames")
    rate = _rational(fps, "fps")
    starts, target = window_starts(n_samples, sample_rate, window_sec, hop_sec, include_tail)
    span = math.ceil(_rational(window_sec, "window_sec") * rate)  # frames one window covers
    q = max(1, span // T)
    rows = []
    for s in starts:
        f = min(n_frames - 1, math.floor(Fraction(s, int(sample_rate)) * rate))
        if frame_grid == "window":
            n = max(1, min(n_frames - f, span))
            rows.append([f + i for i in _even_indices(n, T)])
        else:
            rows.append([min(n_frames - 1, (f // q + j) * q) for j in range(T)])
    frame_idx = torch.tensor(rows, dtype=torch.int32)
    unique, inverse = torch.unique(frame_idx, sorted=True, return_inverse=True)
    return WindowPlan(frame_idx=frame_idx, unique_idx=unique.to(torch.int32), inverse=inverse.to(torch.int32),
                      starts=torch.tensor(starts, dtype=torch.int64),
                      lengths=torch.tensor([min(target, int(n_samples) - s) for s in starts], dtype=torch.int64),
                      starts_sec=[s / int(sample_rate) for s in starts], target=target, window_sec=float(window_sec),
                      frame_grid=frame_grid)
