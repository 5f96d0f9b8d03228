"""Live streaming sessions whose state lives on the device: the counterpart of ``timeline.py`` for input that is
still arriving.

The reference keeps a ``StreamingEmotionSession`` per WebSocket client (``backend/app/streaming.py``): at every tick it
rebuilds the last ``window_seconds`` from host deques, resamples that window on the CPU, encodes its 8 frames again and
runs the model at batch 1.  Here a ``StreamingSessionPool`` holds, for up to ``max_sessions`` clients,

* an audio ring ``[cap]`` fp32 at 16 kHz per session, ``cap = int(max_buffer_seconds * 16000)``: every chunk goes
  through ``clips.ResampleStream`` (mer_resample_stream) once, straight into the ring;
* a preprocessed-frame ring ``[max_frames, 3, 112, 112]`` fp32 per session: every frame is resized and normalised
  once (mer_frames_resize_normalize) into its slot;
* a feature ring ``[max_frames, 512]`` fp32 per session: a frame a window picks is encoded by the trunk once, its
  features stored (mer_rows_scatter), and every later window that picks it gathers them (mer_rows_gather);

and ``infer_ready`` predicts all sessions that are due in one batch.  Memory per session at the defaults: 64 x 147 KiB
of frames (9.2 MiB), 128 KiB of features, 375 KiB of audio.

The host control plane (``StreamState``: timestamps, counts, which slot holds which frame, which slots are encoded,
the frame choice) is pure Python and runs without a device; the device half sits behind ``StreamingSessionPool``.

Rules.  Readiness is the reference's (streaming.py:83-88): at least ``window_seconds`` of audio buffered (counted in
16 kHz samples), at least 2 frames buffered, at least ``step_seconds`` since the last prediction; a single-modality
checkpoint (``audio`` / ``video`` mode) only waits for the modality it reads.  ``add_frame`` drops frames older than
its timestamp minus ``max_buffer_seconds`` (streaming.py:72-75).  A window's audio is the last ``min(buffered,
target)`` samples, zero-padded at the end (preprocess.py:319-323).

Frame choice.  ``frame_grid="window"`` is the reference's: the frames with ``ts >= now - window_seconds`` (all
buffered frames when there are none), ``uniform_indices`` over them (preprocess.py:57-63).  ``frame_grid="shared"``
DEPARTS from it, as the timeline's shared grid does: only frames whose per-session sequence number is a multiple of
``frame_stride`` are eligible, and a window takes the last ``frames_per_window`` eligible frames at or after the
cutoff, repeating its last one when there are fewer (no eligible frame after the cutoff: the eligible frames
buffered; none of those either: the newest frame).  Consecutive windows then share all but the frames that arrived
in between, and the trunk encodes ``1 / frame_stride`` of the stream.

Departures from the reference, all from bounding what its deques leave unbounded:

* a frame beyond ``max_frames`` overwrites the oldest buffered one;
* the audio ring holds exactly ``int(max_buffer_seconds * 16000)`` samples (the reference drops whole chunks);
* a session's sample rate is fixed by its first chunk; a later chunk at another rate raises ``ValueError``;
* the STREAM is resampled once (scipy ``resample_poly``'s filter, chunk-invariant); the reference resamples each
  window, which gives every window its own edge transient.  At 16 kHz input the two are identical.  An output sample
  waits for its newest input: ``10 * max(up, down) / up`` input samples of latency, nothing synthesised at the edge.

Face crops.  ``add_frame(frame, ts, bbox=(x1, y1, x2, y2))`` takes the raw detector box of THAT frame: the frame is
cropped to ``clips.crop_rects`` of it (``crop_with_padding``, the pool's ``pad_ratio``) and resized into its ring slot
in one launch (mer_frames_crop_resize), with the bits of preprocessing the host-cropped frame.  This DEPARTS from the
reference's ``create_session(use_face_crop=True)``, which detects once per window and reuses that box for the
window's frames: here a box belongs to a frame, because a frame is preprocessed once and shared by every window that
picks it.  With a box that is constant over a window the two coincide.  ``bbox=None`` keeps the whole-frame path;
detection itself is the caller's.

A pool and its sessions are driven from one thread and one HIP stream.
"""
from __future__ import annotations

import time
import uuid
from collections import deque
from typing import Any, Deque, Dict, List, Optional, Tuple

import numpy as np
import torch

from .timeline import FRAME_GRIDS, _even_indices

SAMPLE_RATE = 16000


def checked_frame(frame) -> torch.Tensor:
    """A decoded frame (numpy array or tensor) as a uint8 ``[H, W, 3]`` RGB tensor; anything else: ``ValueError``."""
    t = frame
    if isinstance(frame, np.ndarray):  # (a BGR -> RGB view has negative strides: copy it)
        t = torch.from_numpy(np.ascontiguousarray(frame)) if frame.dtype == np.uint8 else None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[-1] != 3 \
            or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("a frame must be uint8 [H, W, 3] (RGB)")
    return t


def checked_chunk(chunk) -> torch.Tensor:
    """An audio chunk (numpy array or tensor of any shape, floating point, samples in [-1, 1]) as a flat fp32 tensor
    (streaming.py:68).  Integer PCM is refused: the reference scales it by 1 / 32768 on the host before the session
    sees it (``decode_pcm16_b64``), and a silent cast would feed the model samples at +-32768."""
    try:
        t = torch.from_numpy(np.ascontiguousarray(chunk)) if isinstance(chunk, np.ndarray) else torch.as_tensor(chunk)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError("an audio chunk must be a floating-point array") from None
    if not t.is_floating_point():
        raise ValueError(f"an audio chunk must hold floating-point samples in [-1, 1], got {t.dtype} (scale PCM16 by "
                         "1 / 32768 first)")
    return t.reshape(-1).to(torch.float32)


class StreamState:
    """Host control plane of one session: no tensors, no device.  Frames are numbered 0, 1, ... as they arrive
    (``seq``); frame ``seq`` lives in ring slot ``seq % max_frames``; ``encoded[slot]`` says whether the feature ring
    holds that slot's features."""

    def __init__(self, window_seconds: float = 3.0, step_seconds: float = 0.5, max_buffer_seconds: float = 6.0,
                 frames_per_window: int = 8, max_frames: int = 64, frame_grid: str = "window",
                 frame_stride: Optional[int] = None, need_frames: bool = True, need_audio: bool = True):
        if frame_grid not in FRAME_GRIDS:
            raise ValueError(f"unknown frame_grid {frame_grid!r}: one of {FRAME_GRIDS}")
        if not (float(window_seconds) > 0 and float(step_seconds) >= 0 and float(max_buffer_seconds) > 0):
            raise ValueError("window_seconds and max_buffer_seconds must be positive, step_seconds >= 0")
        if float(max_buffer_seconds) < float(window_seconds):
            raise ValueError(f"max_buffer_seconds {max_buffer_seconds} is shorter than one window of {window_seconds} s")
        if int(frames_per_window) < 1:
            raise ValueError(f"frames_per_window must be at least 1, got {frames_per_window}")
        if int(max_frames) < int(frames_per_window):
            raise ValueError(f"max_frames {max_frames} < frames_per_window {frames_per_window}: one window would not "
                             "fit its own frames")
        if frame_grid == "shared":
            if frame_stride is None or int(frame_stride) < 1:
                raise ValueError("frame_grid='shared' needs frame_stride >= 1 (every frame_stride-th frame is eligible)")
        self.window_seconds, self.step_seconds = float(window_seconds), float(step_seconds)
        self.max_buffer_seconds = float(max_buffer_seconds)
        self.frames_per_window, self.max_frames = int(frames_per_window), int(max_frames)
        self.frame_grid, self.frame_stride = frame_grid, int(frame_stride or 1)
        self.need_frames, self.need_audio = bool(need_frames), bool(need_audio)
        self.target = max(1, int(SAMPLE_RATE * self.window_seconds))  # samples per window
        self.cap = max(self.target, int(SAMPLE_RATE * self.max_buffer_seconds))  # samples the audio ring holds
        self.frames: Deque[Tuple[float, int]] = deque()  # (timestamp, seq), oldest first
        self.encoded = [False] * self.max_frames
        self.next_seq = 0
        self.audio = None  # clips.ResampleCount (inputs consumed, 16 kHz samples emitted), made by the first chunk
        self.last_prediction_ts = 0.0

    # ---- frames
    def add_frame(self, timestamp: float) -> int:
        """Register the next frame; returns its ring slot (the caller writes the pixels there)."""
        now = float(timestamp)
        if len(self.frames) == self.max_frames:  # the bounded ring: the new frame takes the oldest one's slot
            self.frames.popleft()
        seq = self.next_seq
        self.next_seq += 1
        slot = seq % self.max_frames
        self.frames.append((now, seq))
        self.encoded[slot] = False
        cutoff = now - self.max_buffer_seconds
        while self.frames and self.frames[0][0] < cutoff:
            self.frames.popleft()
        return slot

    def slot_of(self, seq: int) -> int:
        return seq % self.max_frames

    # ---- audio
    def check_rate(self, sample_rate) -> int:
        sr = int(sample_rate)
        if sr <= 0:
            raise ValueError(f"sample_rate must be positive, got {sample_rate!r}")
        if self.audio is not None and sr != self.audio.sr_in:
            raise ValueError(f"this session's audio arrives at {self.audio.sr_in} Hz (its first chunk); got a chunk at "
                             f"{sr} Hz")
        return sr

    def open_audio(self, sample_rate):
        """The session's audio counts, made at the first chunk's rate.  The one host copy of them: the device
        resampler advances this object at every push; ``add_audio`` advances it where nothing is resampled."""
        from .clips import ResampleCount

        sr = self.check_rate(sample_rate)
        if self.audio is None:
            self.audio = ResampleCount(sr, SAMPLE_RATE)
        return self.audio

    def add_audio(self, n_samples: int, sample_rate) -> int:
        """Register ``n_samples`` more inputs at ``sample_rate``; returns how many 16 kHz samples they emit."""
        return self.open_audio(sample_rate).advance(n_samples)

    @property
    def sample_rate(self) -> Optional[int]:
        return None if self.audio is None else self.audio.sr_in

    @property
    def n_in(self) -> int:
        return 0 if self.audio is None else self.audio.n_in

    @property
    def n_out(self) -> int:
        return 0 if self.audio is None else self.audio.n_out

    @property
    def audio_buffered(self) -> int:
        return min(self.n_out, self.cap)

    # ---- cadence
    def ready(self, now: float) -> bool:
        enough_audio = not self.need_audio or self.audio_buffered >= int(SAMPLE_RATE * self.window_seconds)
        enough_frames = not self.need_frames or len(self.frames) >= 2
        return enough_audio and enough_frames and (float(now) - self.last_prediction_ts) >= self.step_seconds

    def select(self, now: float) -> Tuple[List[int], int]:
        """``(seqs, n_window_frames)``: the ``frames_per_window`` frames (by sequence number) the window ending at
        ``now`` shows, and how many buffered frames that window covers."""
        if not self.frames:
            raise ValueError("no frame buffered")
        cutoff = float(now) - self.window_seconds
        window = [q for ts, q in self.frames if ts >= cutoff] or [q for _, q in self.frames]
        T = self.frames_per_window
        if self.frame_grid == "window":
            return [window[i] for i in _even_indices(len(window), T)], len(window)
        s = self.frame_stride
        cand = [q for q in window if q % s == 0] or [q for _, q in self.frames if q % s == 0] or [self.frames[-1][1]]
        cand = cand[-T:]
        return cand + [cand[-1]] * (T - len(cand)), len(window)

    def audio_window(self) -> Tuple[int, int]:
        """``(end, count)`` of ``kernels.ring_windows``: the ring position after the newest sample, samples held."""
        return self.n_out % self.cap, self.audio_buffered


class StreamingSession:
    """One client's stream, with the reference's surface (streaming.py:55-117).  Made by
    ``StreamingSessionPool.create_session``."""

    def __init__(self, pool, slot: int, state: StreamState, session_id: Optional[str] = None):
        self.pool, self.slot, self.state = pool, int(slot), state
        self.session_id = session_id or uuid.uuid4().hex
        self.resampler = None  # clips.ResampleStream, made by the first chunk

    @property
    def last_prediction_ts(self) -> float:
        return self.state.last_prediction_ts

    def add_frame(self, frame, timestamp: Optional[float] = None, bbox=None) -> None:
        """A decoded RGB frame, uint8 ``[H, W, 3]`` (numpy or tensor, host or device): preprocessed once into its
        ring slot.  A frame beyond ``max_frames`` overwrites the oldest; frames older than ``timestamp -
        max_buffer_seconds`` are dropped.  ``bbox``: this frame's raw face box ``(x1, y1, x2, y2)``; the frame is
        cropped to the padded box on the device (an empty box: the whole frame).  A malformed box is a ``ValueError``
        before anything is stored."""
        t = checked_frame(frame)
        now = float(timestamp if timestamp is not None else time.monotonic())
        pool = self._open_pool()
        if bbox is None:
            pool._store_frame(self, t, now)
            return
        from .clips import crop_rects

        pool._store_frame(self, t, now, crop_rects(t.shape[0], t.shape[1], [bbox], pool.pad_ratio)[0])

    def add_audio_chunk(self, chunk, sample_rate: int, timestamp: Optional[float] = None) -> None:
        """Mono samples at ``sample_rate`` (the rate of the session's first chunk): resampled once into the audio
        ring.  ``timestamp`` is accepted and unused, as in the reference."""
        sr = self.state.check_rate(sample_rate)
        flat = checked_chunk(chunk)
        if flat.numel():
            self._open_pool()._store_audio(self, flat, sr)

    def ready_for_inference(self, now: Optional[float] = None) -> bool:
        return self.state.ready(float(now if now is not None else time.monotonic()))

    def infer(self, now: Optional[float] = None) -> Dict[str, Any]:
        """Predict this session's last window now, whatever the cadence says (streaming.py:103-117)."""
        now = float(now if now is not None else time.monotonic())
        return self._open_pool()._infer([self], now)[self.session_id]

    def _open_pool(self):
        if self.pool is None:
            raise RuntimeError(f"streaming session {self.session_id} is closed")
        return self.pool


class StreamingSessionPool:
    """``max_sessions`` streaming sessions on one runner; see the module docstring.  ``infer_ready(now)`` predicts
    every session that is due in one batch: the union of their selected, not yet encoded frames goes through the trunk
    (at most ``max_windows_per_batch * frames_per_window`` frames per call), one ``forward_from_frame_features`` call
    per ``max_windows_per_batch`` sessions, one device-to-host copy.  There is no CPU fallback."""

    def __init__(self, runner, max_sessions: int, window_seconds: float = 3.0, step_seconds: float = 0.5,
                 max_buffer_seconds: float = 6.0, frames_per_window: int = 8, max_frames: int = 64,
                 frame_grid: str = "window", frame_stride: Optional[int] = None, max_windows_per_batch: int = 64,
                 pad_ratio: float = 0.3):
        if runner.device.type != "cuda":
            raise RuntimeError("a streaming session pool runs on the MI355X kernels; build the runner on a GPU device "
                               "(device='cuda')")
        if int(max_sessions) < 1:
            raise ValueError(f"max_sessions must be at least 1, got {max_sessions}")
        if int(max_windows_per_batch) < 1:
            raise ValueError(f"max_windows_per_batch must be at least 1, got {max_windows_per_batch}")
        self.runner, self.pad_ratio = runner, float(pad_ratio)  # pad_ratio: the face crop's (add_frame's bbox)
        self.use_video, self.use_audio = runner.fusion_mode != "audio", runner.fusion_mode != "video"
        self._kw = dict(window_seconds=window_seconds, step_seconds=step_seconds, max_buffer_seconds=max_buffer_seconds,
                        frames_per_window=frames_per_window, max_frames=max_frames, frame_grid=frame_grid,
                        frame_stride=frame_stride, need_frames=self.use_video, need_audio=self.use_audio)
        proto = StreamState(**self._kw)  # argument errors before any device work
        self.max_sessions, self.max_frames, self.T = int(max_sessions), proto.max_frames, proto.frames_per_window
        self.cap, self.target, self.window_seconds = proto.cap, proto.target, proto.window_seconds
        self.frame_size, self.chunk_w = 112, int(max_windows_per_batch)  # the trunk's input size
        dev = runner.device
        self.audio_rings = torch.zeros(self.max_sessions, self.cap, device=dev) if self.use_audio else None
        self.frame_ring = self.feature_ring = None
        if self.use_video:
            vnet = runner.model if runner.fusion_mode == "video" else runner.model.video_model
            self._vnet, self.embedding_dim = vnet, int(vnet.embedding_dim)
            rows = self.max_sessions * self.max_frames
            self.frame_ring = torch.zeros(rows, 3 * self.frame_size * self.frame_size, device=dev)
            self.feature_ring = torch.zeros(rows, self.embedding_dim, device=dev)
        self.sessions: Dict[str, StreamingSession] = {}
        self._free = list(range(self.max_sessions - 1, -1, -1))
        self.stats = dict(frames_added=0, frames_encoded=0, trunk_batches=0, predictions=0, audio_samples_resampled=0)
        self.debug = False
        self.last_assembly: Dict[str, Any] = {}  # with debug: what the last _infer assembled

    # ---- sessions
    def create_session(self) -> StreamingSession:
        if not self._free:
            raise RuntimeError(f"all {self.max_sessions} session slots are in use")
        s = StreamingSession(self, self._free.pop(), StreamState(**self._kw))
        self.sessions[s.session_id] = s
        return s

    def close_session(self, session_id: str) -> None:
        """Forget the session and free its slot; the next session in that slot starts from empty rings (its counts
        and flags are new: nothing of the old rings' contents is ever selected)."""
        s = self.sessions.pop(session_id, None)
        if s is not None:
            s.pool = None
            self._free.append(s.slot)

    def infer_ready(self, now: Optional[float] = None) -> Dict[str, Dict[str, Any]]:
        now = float(now if now is not None else time.monotonic())
        due = [s for s in self.sessions.values() if s.state.ready(now)]
        return self._infer(due, now) if due else {}

    # ---- device half
    def _store_frame(self, s: StreamingSession, frame: torch.Tensor, now: float, rect=None) -> None:
        from . import clips

        slot = s.state.add_frame(now)
        self.stats["frames_added"] += 1
        if not self.use_video:
            return
        dev = self.runner.device
        frame = frame.to(dev) if frame.is_cuda else clips._h2d(frame.contiguous(), dev)
        row = self.frame_ring[s.slot * self.max_frames + slot].view(1, 3, self.frame_size, self.frame_size)
        if rect is None:
            clips.preprocess_frames(frame[None], self.frame_size, out=row)
        else:  # the frame's own padded face box, cropped and resized in one launch
            H, W, _ = frame.shape
            clips.crop_resize_frames(frame.contiguous().view(-1), clips.crop_rows([0], H, W, rect[None]),
                                     self.frame_size, out=row)

    def _store_audio(self, s: StreamingSession, flat: torch.Tensor, sr: int) -> None:
        from . import clips

        if not self.use_audio:  # a video checkpoint: the samples are counted, nothing is resampled
            s.state.add_audio(int(flat.numel()), sr)
            return
        if s.resampler is None:  # the resampler advances the session's own counts
            s.resampler = clips.ResampleStream(sr, self.audio_rings[s.slot], SAMPLE_RATE, count=s.state.open_audio(sr))
        s.resampler.push(flat)
        self.stats["audio_samples_resampled"] += int(flat.numel())

    def _infer(self, sessions: List[StreamingSession], now: float) -> Dict[str, Dict[str, Any]]:
        from . import clips
        from . import kernels as K
        from .optimized_runtime import _result_row, _softmax

        r, mode, B, T = self.runner, self.runner.fusion_mode, len(sessions), self.T
        with torch.inference_mode():
            v_feat = audio = None
            picks = []
            if self.use_video:
                need, rows, owner = [], [], {}  # need: ring rows to encode, in first-use order, each once
                for s in sessions:
                    seqs, n_win = s.state.select(now)
                    picks.append((seqs, n_win))
                    base = s.slot * self.max_frames
                    for q in seqs:
                        slot = s.state.slot_of(q)
                        rows.append(base + slot)
                        if not s.state.encoded[slot] and base + slot not in owner:
                            owner[base + slot] = (s.state, slot)
                            need.append(base + slot)
                if need:
                    S = self.frame_size
                    x = K.rows_gather(self.frame_ring, need).view(-1, 3, S, S)
                    step = self.chunk_w * T
                    feats = [self._vnet.backbone(x[i:i + step]).reshape(-1, self.embedding_dim)
                             for i in range(0, len(need), step)]
                    feats = feats[0] if len(feats) == 1 else torch.cat(feats)
                    K.rows_scatter(feats.float(), need, self.feature_ring)
                    for state, slot in owner.values():
                        state.encoded[slot] = True
                    self.stats["frames_encoded"] += len(need)
                    self.stats["trunk_batches"] += len(range(0, len(need), step))
                v_feat = K.rows_gather(self.feature_ring, rows).view(B, T, self.embedding_dim)
            else:
                picks = [([], len(s.state.frames)) for s in sessions]
            counts = [0] * B
            if self.use_audio:
                meta = [s.state.audio_window() for s in sessions]
                counts = [min(c, self.target) for _, c in meta]
                wav = K.ring_windows(self.audio_rings, [s.slot for s in sessions], [e for e, _ in meta],
                                     [c for _, c in meta], self.target)
                audio = clips.log_mel(wav, n_mels=r.n_mels) if r.uses_mel else wav
            out_rows = []
            for i in range(0, B, self.chunk_w):
                j = i + self.chunk_w
                if mode == "audio":
                    out = r.model(audio[i:j])
                elif mode == "video":
                    out = r.model.forward_from_frame_features(v_feat[i:j])
                else:
                    out = r.model.forward_from_frame_features(v_feat[i:j], audio[i:j])
                out_rows.append(out.contiguous().float() if mode == "late" else _softmax(out))
            probs = out_rows[0] if len(out_rows) == 1 else torch.cat(out_rows)
            if self.debug:
                self.last_assembly = dict(sessions=[s.session_id for s in sessions], seqs=[p[0] for p in picks],
                                          rows=rows if self.use_video else [], v_feat=v_feat,
                                          waveforms=wav if self.use_audio else None, probs=probs)
            host = probs.cpu()  # the one device-to-host copy
        results = {}
        for b, s in enumerate(sessions):
            s.state.last_prediction_ts = now
            d = _result_row(r, host[b])
            d["session_id"], d["window_seconds"] = s.session_id, self.window_seconds
            d["num_buffered_frames"], d["num_audio_samples"] = picks[b][1], counts[b]
            results[s.session_id] = d
        self.stats["predictions"] += B
        return results

    def debug_frames(self, session_id: str):
        """``(seqs, rows)``: the buffered frames' sequence numbers, oldest first, and their preprocessed-frame ring
        rows ``[n, 3, S, S]`` (a copy)."""
        s = self.sessions[session_id]
        seqs = [q for _, q in s.state.frames]
        if not self.use_video or not seqs:
            return seqs, None
        idx = torch.tensor([s.slot * self.max_frames + s.state.slot_of(q) for q in seqs], device=self.runner.device)
        return seqs, self.frame_ring[idx].view(-1, 3, self.frame_size, self.frame_size)
