"""Clip assembly on the MI355X (first step): the arithmetic of ``src/data/ravdess.py``'s
``load_video_frames`` after decode and ``load_audio_wav`` after ``librosa.load``, run on the device so only
decoded uint8 frames / raw waveforms cross PCIe and the batch is assembled in HBM.

* ``preprocess_frames`` -- decoded RGB uint8 frames ``[N, H, W, 3]`` -> ``[N, 3, size, size]`` fp32:
  ``cv2.resize(..., INTER_LINEAR)`` (ravdess.py:352), ``/ 255`` (:363), ImageNet normalisation (:386-389).
* ``video_clip_batch`` -- ``B`` clips of ``T`` such frames -> the model's ``[B, T, 3, size, size]`` input.
* ``augment_clips`` -- the train-split video augmentation (ravdess.py:366-384: uint8 round trip,
  ``cv2.GaussianBlur(k, 0)``, darken, Gaussian noise, clip) + normalisation of ``B`` clips, per-clip draws from
  ``draw_video_augment``.
* ``pad_crop_waveforms`` -- a ragged list of mono waveforms -> ``[B, 1, sample_rate * duration]``
  (ravdess.py:505-513).

* ``log_mel`` -- a waveform batch -> the log-mel spectrogram ``[B, 1, n_mels, T]`` of ``load_audio_mel``
  (ravdess.py:478-485: ``MelSpectrogram(16000, n_mels=64, win_length=400, hop_length=160)`` + ``AmplitudeToDB()``).

* ``gather_preprocess_frames`` / ``waveform_windows`` -- the same two steps for the overlapping windows of one long
  recording (``timeline.py``): frames picked by index out of the decoded recording, audio windows as offsets into it.

* ``ResampleStream`` -- a live stream resampled once, chunk by chunk, into a device ring (``streaming.py``; the
  windows come out of the rings through ``kernels.ring_windows``).

* ``resample_clips`` / ``mix_noise_clips`` / ``assemble_waveforms`` -- ``load_audio_wav`` after the decode for a whole
  batch: ragged clips at their native rates resampled (the stream's arithmetic, bit for bit), padded / cropped and
  mixed with the bar-noise track at the drawn SNR (``draw_audio_augment``: the host's draws in the host's order).

* ``crop_rects`` / ``pack_frames`` / ``crop_resize_frames`` -- the face-box crop (face_crop.py:151-190) and the resize
  in one ragged launch: images of differing sizes in one buffer, one rectangle per output frame, the bits of resizing
  the host-cropped copy.  ``gather_preprocess_frames(..., rects=)``, the streaming sessions' ``add_frame(bbox=)`` and
  ``ClipLoader(device_video=True)`` run on it.

Decoding (cv2.VideoCapture / librosa) and face detection stay on the host, and so does the audio path of the
default ``ClipLoader``.  Kernels: ``csrc/clips.hip``, ``csrc/mel.hip``, ``csrc/timeline.hip``,
``csrc/stream.hip``, ``csrc/audio_clips.hip``, ``csrc/frame_crop.hip``;
CPU restatements:
``oracle/clips_ref.py``, ``tests/mel_ref.py``.
"""
from __future__ import annotations

import math
from typing import List, Sequence

import torch

from . import kernels as K

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def preprocess_frames(frames: torch.Tensor, size: int = 112, out: torch.Tensor = None) -> torch.Tensor:
    """``[N, H, W, 3]`` uint8 RGB on the GPU -> ``[N, 3, size, size]`` fp32, normalised (into ``out`` when given: the
    streaming sessions' frame-ring slots)."""
    if not frames.is_cuda:
        raise RuntimeError("preprocess_frames runs on the MI355X kernels; move the frames to the GPU")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("frames must be uint8 [N, H, W, 3] (RGB)")
    frames = frames.contiguous()
    N, H, W, _ = frames.shape
    if out is None:
        out = torch.empty(N, 3, size, size, device=frames.device, dtype=torch.float32)
    elif tuple(out.shape) != (N, 3, size, size) or out.dtype != torch.float32 or not out.is_contiguous() \
            or out.device != frames.device:
        raise ValueError(f"preprocess_frames out must be contiguous fp32 [{N}, 3, {size}, {size}] on {frames.device}")
    K.LIB("mer_frames_resize_normalize", N, H, W, frames.data_ptr(), H * W * 3, size, *IMAGENET_MEAN, *IMAGENET_STD,
          out.data_ptr(), K.stream_ptr())
    return out


def gather_preprocess_frames(frames: torch.Tensor, idx, size: int = 112, rects=None) -> torch.Tensor:
    """``preprocess_frames(frames.index_select(0, idx), size)``, bit for bit, without the gathered uint8 copy: output
    ``n`` is made from frame ``idx[n]`` of the decoded recording ``[N, H, W, 3]`` (repeats and any order allowed), one
    launch for all of them.  ``idx``: a sequence or an int32 / int64 tensor; every value is checked against ``[0, N)``
    on the host (``ValueError``) before anything is launched.

    ``rects``: one final rectangle ``(x1, y1, x2, y2)`` per output (``crop_rects``); output ``n`` is then the
    preprocessing of ``frames[idx[n], y1:y2, x1:x2]``, through ``crop_resize_frames``.  ``None`` keeps the entry point
    and the bits this function always had."""
    if not frames.is_cuda:
        raise RuntimeError("gather_preprocess_frames runs on the MI355X kernels; move the frames to the GPU")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("frames must be uint8 [N, H, W, 3] (RGB)")
    frames = frames.contiguous()
    N, H, W, _ = frames.shape
    if rects is not None:
        host = torch.as_tensor(idx)
        if host.numel() == 0 and host.dim() == 1:
            host = host.to(torch.int64)
        if host.dtype not in (torch.int32, torch.int64) or host.dim() != 1:
            raise ValueError(f"frame index must be a 1-D int32 / int64 array, got {host.dtype} {tuple(host.shape)}")
        host = host.cpu().to(torch.int64)
        if host.numel() and (int(host.min()) < 0 or int(host.max()) >= N):
            raise ValueError(f"frame index outside [0, {N}): min {int(host.min())}, max {int(host.max())}")
        rows = crop_rows(host * (H * W * 3), H, W, rects)
        return crop_resize_frames(frames.view(-1), rows, size)
    dix = K.checked_index(idx, N, frames.device, "frame index")
    U = dix.numel()
    out = torch.empty(U, 3, size, size, device=frames.device, dtype=torch.float32)
    if U:
        K.LIB("mer_frames_gather_resize_normalize", N, H, W, frames.data_ptr(), H * W * 3, U, dix.data_ptr(), size,
              *IMAGENET_MEAN, *IMAGENET_STD, out.data_ptr(), K.stream_ptr())
    return out


CROP_MAX_SIDE = 1 << 24  # csrc/frame_crop.hip keeps W * 3 and the tap offsets inside an int
CROP_MAX_SIZE = 16 * 65535  # its grid holds one band of 16 output rows per y block


def _int_table(a, cols: int, what: str):
    """``a`` as a host int64 numpy array ``[n, cols]``; anything that is not an integer array of that shape:
    ``ValueError``."""
    import numpy as np

    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    try:
        t = np.asarray(a)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be an integer array [n, {cols}]") from None
    if t.size == 0 and t.ndim <= 2:
        t = t.reshape(0, cols).astype(np.int64)
    if t.dtype.kind not in "iu" or t.ndim != 2 or t.shape[1] != cols:
        raise ValueError(f"{what} must be an integer array [n, {cols}], got {t.dtype} {tuple(t.shape)}")
    return t.astype(np.int64)


def crop_rects(H: int, W: int, boxes, pad_ratio: float = 0.3):
    """Raw detector boxes ``(x1, y1, x2, y2)`` of ``H x W`` frames -> the rectangles the frames are cropped to, host
    int64 ``[n, 4]``, half-open as ``frame[y1:y2, x1:x2]``: ``crop_with_padding``'s box (face_crop.py:151-190, each
    side padded by ``int(side * pad_ratio)``, clipped to the frame) through ``data.face_crop_box``.  ``boxes``: a
    sequence of boxes, an integer array ``[n, 4]``, and ``None`` in place of a box where nothing was detected.  A
    missing box, or a rectangle that comes out empty (``x2 <= x1`` or ``y2 <= y1``), means the whole frame ``(0, 0, W,
    H)`` -- ``data.select_frames``'s rule.  Host only: no device is touched."""
    import numpy as np

    from .data import face_crop_box

    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"frame size must be positive, got {H} x {W}")
    boxes = list(boxes) if not isinstance(boxes, (np.ndarray, torch.Tensor)) else _int_table(boxes, 4, "boxes")
    out = np.empty((len(boxes), 4), dtype=np.int64)
    for n, b in enumerate(boxes):
        rect = (0, 0, W, H)
        if b is not None:
            try:
                vals = [int(v) for v in b]
                exact = all(int(v) == v for v in b)
            except (TypeError, ValueError):
                raise ValueError(f"box {n} must be four integers (x1, y1, x2, y2), got {b!r}") from None
            if len(vals) != 4 or not exact or any(abs(v) >= 2 ** 30 for v in vals):
                raise ValueError(f"box {n} must be four integers (x1, y1, x2, y2) below 2^30, got {b!r}")
            x1, y1, x2, y2 = face_crop_box(H, W, vals, pad_ratio)
            if x2 > x1 and y2 > y1:
                rect = (x1, y1, x2, y2)
        out[n] = rect
    return out


def crop_rows(offsets, H, W, rects):
    """The descriptor table of ``crop_resize_frames``, host int64 ``[n, 8]``: row ``n`` = ``{offsets[n], H[n], W[n],
    x1, y1, x2, y2, 0}``.  ``H`` / ``W``: one int for all rows or one per row; ``rects`` ``[n, 4]``."""
    import numpy as np

    rects = _int_table(rects, 4, "rects")
    n = rects.shape[0]
    rows = np.zeros((n, 8), dtype=np.int64)
    if isinstance(offsets, torch.Tensor):
        offsets = offsets.cpu().numpy()
    try:
        if np.size(offsets) != n:
            raise ValueError
        rows[:, 0] = np.asarray(offsets, dtype=np.int64).reshape(-1)
        rows[:, 1], rows[:, 2] = np.asarray(H, dtype=np.int64), np.asarray(W, dtype=np.int64)
    except (TypeError, ValueError):
        raise ValueError(f"crop_rows: {n} rectangles need {n} offsets and one or {n} heights / widths") from None
    rows[:, 3:7] = rects
    return rows


def pack_frames(arrays, device="cuda"):
    """Decoded frames of differing sizes -> one device byte buffer: ``arrays`` is a list of uint8 host arrays (numpy or
    tensors) ``[T_i, H_i, W_i, 3]``; every image is copied once into ONE pinned staging buffer, tightly packed in list
    order (``stage_frames``), which crosses PCIe in one asynchronous copy (``_h2d``'s pinned route: the caching host
    allocator keeps the block until the copy has run).  Returns ``(buffer, offsets)``: the 1-D uint8 device tensor and
    the byte offset of every image, ``sum(T_i)`` ints in order."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("pack_frames stages frames for the MI355X kernels; pass device='cuda'")
    stage, offsets = stage_frames(arrays)
    return stage.to(dev, non_blocking=True), offsets


def stage_frames(arrays):
    """The host half of ``pack_frames``: ``(pinned 1-D uint8 host tensor, byte offset of every image)``.  A loader
    calls it on its producer thread, so the gather into pinned memory stays off the thread that feeds the device."""
    import numpy as np

    flat, offsets, total = [], [], 0
    for a in arrays:
        t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        if not isinstance(t, torch.Tensor) or t.is_cuda or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3:
            raise ValueError("pack_frames takes uint8 host arrays [T, H, W, 3] (RGB)")
        T, H, W, _ = t.shape
        offsets += [total + i * H * W * 3 for i in range(T)]
        total += T * H * W * 3
        flat.append(t.contiguous().view(-1))
    if not total:
        raise ValueError("pack_frames: no pixels to pack")
    stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    torch.cat(flat, out=stage)
    return stage, offsets


def crop_resize_frames(buffer: torch.Tensor, rows, size: int = 112, u8: bool = False,
                       out: torch.Tensor = None) -> torch.Tensor:
    """Ragged crop-and-resize, one launch (mer_frames_crop_resize): ``buffer`` is a 1-D uint8 device tensor of tightly
    packed RGB images (``pack_frames``, or a decoded recording viewed flat), ``rows`` the host int64 table ``[n, 8]``
    of ``crop_rows`` (``[n, 7]`` is taken too): image byte offset, ``H0``, ``W0`` and the final half-open rectangle
    ``(x1, y1, x2, y2)``.  Output ``n`` is ``preprocess_frames`` (``u8=True``: ``resize_frames_u8``) of the contiguous
    copy of ``image[y1:y2, x1:x2]``, bit for bit: fp32 ``[n, 3, size, size]`` or uint8 ``[n, size, size, 3]``, written
    into ``out`` when given.  Every row is checked against the buffer on the host (``ValueError``) before the table is
    uploaded; images may repeat and overlap."""
    import numpy as np

    size = int(size)
    if not 1 <= size <= CROP_MAX_SIZE:
        raise ValueError(f"size must be in [1, {CROP_MAX_SIZE}], got {size}")
    if not isinstance(buffer, torch.Tensor) or buffer.dtype != torch.uint8 or buffer.dim() != 1 \
            or not buffer.is_contiguous():
        raise ValueError("buffer must be a contiguous 1-D uint8 tensor")
    t = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    if t.ndim == 2 and t.shape[1] == 7 and t.dtype.kind in "iu":
        t = np.concatenate([t, np.zeros((t.shape[0], 1), dtype=t.dtype)], axis=1)
    t = _int_table(t, 8, "rows")
    n, nbytes = int(t.shape[0]), int(buffer.numel())
    if n >= 2 ** 31:
        raise ValueError(f"{n} output frames do not fit one call")
    if n:
        off, H0, W0, x1, y1, x2, y2, last = (t[:, c] for c in range(8))
        if int(H0.min()) < 1 or int(W0.min()) < 1 or int(H0.max()) > CROP_MAX_SIDE or int(W0.max()) > CROP_MAX_SIDE:
            raise ValueError(f"image sizes must be in [1, {CROP_MAX_SIDE}]")
        bad = (off < 0) | (off + H0 * W0 * 3 > nbytes) | (x1 < 0) | (y1 < 0) | (x2 <= x1) | (y2 <= y1) | (x2 > W0) \
            | (y2 > H0) | (last != 0)
        if bool(bad.any()):
            b = int(np.argmax(bad))
            raise ValueError(f"row {b} {t[b].tolist()}: the image must lie inside the buffer of {nbytes} bytes and the "
                             "rectangle, non-empty, inside the image (last column 0)")
    if not buffer.is_cuda:
        raise RuntimeError("crop_resize_frames runs on the MI355X kernels; move the buffer to the GPU")
    dev = buffer.device
    shape = (n, size, size, 3) if u8 else (n, 3, size, size)
    dtype = torch.uint8 if u8 else torch.float32
    if out is None:
        out = torch.empty(shape, device=dev, dtype=dtype)
    elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"crop_resize_frames out must be contiguous {dtype} {list(shape)} on {dev}")
    if n:
        desc = _h2d(torch.from_numpy(np.ascontiguousarray(t)), dev)
        K.LIB("mer_frames_crop_resize", buffer.data_ptr(), nbytes, n, desc.data_ptr(), size, int(bool(u8)),
              *IMAGENET_MEAN, *IMAGENET_STD, out.data_ptr(), K.stream_ptr())
    return out


def video_clip_batch(frames: torch.Tensor, size: int = 112) -> torch.Tensor:
    """``[B, T, H, W, 3]`` uint8 -> ``[B, T, 3, size, size]`` fp32 (the FusionModel video input)."""
    B, T = frames.shape[:2]
    return preprocess_frames(frames.reshape(B * T, *frames.shape[2:]), size).view(B, T, 3, size, size)


NORMAL_TABLE_BITS = 16


def normal_table() -> torch.Tensor:
    """fp32 [65536]: the standard normal inverse CDF at (i + 0.5) / 65536 (float64, then rounded) -- the
    augmentation noise draws z = table[hash >> 16] (a 16-bit-resolution Gaussian, |z| <= 4.17)."""
    n = 1 << NORMAL_TABLE_BITS
    u = (torch.arange(n, dtype=torch.float64) + 0.5) / n
    return torch.special.ndtri(u).to(torch.float32)


_ZTABLES = {}


def _ztable(dev) -> torch.Tensor:
    t = _ZTABLES.get(dev)
    if t is None:
        t = _ZTABLES[dev] = normal_table().to(dev)
    return t


def draw_video_augment(rng) -> tuple:
    """One clip's draws of ravdess.py:368-372 from a numpy Generator, in the reference's order: brightness factor
    U(0.2, 0.6), noise scale U(0, 5e-4), blur ksize from {3, 5, 7} -- plus the 63-bit seed of the clip's noise."""
    factor = float(rng.uniform(0.2, 0.6))
    noise_scale = float(rng.uniform(0.0, 0.0005))
    ksize = int(rng.choice([3, 5, 7]))
    if ksize % 2 == 0:
        ksize += 1
    return factor, noise_scale, ksize, int(rng.integers(0, 2 ** 63 - 1))


def resize_frames_u8(frames: torch.Tensor, size: int = 112, out: torch.Tensor = None) -> torch.Tensor:
    """``[N, H, W, 3]`` uint8 on the GPU -> ``[N, size, size, 3]`` uint8 (cv2.resize INTER_LINEAR, ravdess.py:352)."""
    if not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("frames must be uint8 [N, H, W, 3] (RGB) on the GPU")
    frames = frames.contiguous()
    N, H, W, _ = frames.shape
    if out is None:
        out = torch.empty(N, size, size, 3, device=frames.device, dtype=torch.uint8)
    K.LIB("mer_frames_resize_u8", N, H, W, frames.data_ptr(), H * W * 3, size, out.data_ptr(), K.stream_ptr())
    return out


def augment_clips(frames_u8: torch.Tensor, params: Sequence[tuple]) -> torch.Tensor:
    """Resized clips ``[B, T, S, S, 3]`` uint8 on the GPU + one ``draw_video_augment`` tuple per clip ->
    ``[B, T, 3, S, S]`` fp32: the augmentation of ravdess.py:366-384 then the ImageNet normalisation (:386-389)."""
    if not frames_u8.is_cuda:
        raise RuntimeError("augment_clips runs on the MI355X kernels; move the frames to the GPU")
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 5 or frames_u8.shape[-1] != 3 \
            or frames_u8.shape[2] != frames_u8.shape[3]:
        raise ValueError("frames must be uint8 [B, T, S, S, 3]")
    B, T, S = frames_u8.shape[:3]
    if len(params) != B:
        raise ValueError(f"{len(params)} augmentation draws for {B} clips")
    for _, _, k, _ in params:
        if k not in (1, 3, 5, 7):
            raise ValueError(f"blur ksize {k}: the device blur implements cv2's sigma-0 kernels of size <= 7")
    dev = frames_u8.device
    fp = _h2d(torch.tensor([[f, n, float(k)] for f, n, k, _ in params], dtype=torch.float32), dev)
    seeds = _h2d(torch.tensor([sd for _, _, _, sd in params], dtype=torch.int64), dev)
    out = torch.empty(B, T, 3, S, S, device=dev, dtype=torch.float32)
    K.LIB("mer_frames_augment_normalize", B * T, S, T, frames_u8.contiguous().data_ptr(), fp.data_ptr(),
          seeds.data_ptr(), _ztable(dev).data_ptr(), *IMAGENET_MEAN, *IMAGENET_STD, out.data_ptr(), K.stream_ptr())
    return out


def _h2d(t: torch.Tensor, dev) -> torch.Tensor:
    """Asynchronous host-to-device copy from a PINNED staging copy: the caching host allocator keeps the pinned
    block alive until the copy has executed.  (An asynchronous copy straight from a pageable temporary may still be
    in flight when the temporary is freed and its memory reused -- the device then reads whatever is there.)"""
    return t.pin_memory().to(dev, non_blocking=True)


def pad_crop_waveforms(wavs: Sequence[torch.Tensor], sample_rate: int = 16000, duration_sec: float = 3.0,
                       device=None) -> torch.Tensor:
    """Ragged mono waveforms (1-D fp32, host or device) -> ``[B, 1, target]`` on the GPU, zero-padded at the end or
    cropped to ``target = int(sample_rate * duration_sec)`` (ravdess.py:505-513)."""
    if not wavs:
        raise ValueError("empty waveform batch")
    target = int(sample_rate * duration_sec)
    dev = torch.device(device) if device is not None else next((w.device for w in wavs if w.is_cuda), None)
    if dev is None or dev.type != "cuda":
        raise RuntimeError("pad_crop_waveforms assembles the batch on the MI355X; pass device='cuda'")
    flat: List[torch.Tensor] = [w.reshape(-1).to(torch.float32) for w in wavs]
    lengths = [int(w.numel()) for w in flat]
    offsets = [0]
    for n in lengths[:-1]:
        offsets.append(offsets[-1] + n)
    if not sum(lengths):
        packed = torch.zeros(1, device=dev)
    elif all(not w.is_cuda for w in flat):  # decoded on the host: one contiguous PINNED host buffer, one H2D copy
        packed = _h2d(torch.cat(flat), dev)
    else:
        packed = torch.cat([w.to(dev) if w.is_cuda else _h2d(w, dev) for w in flat])
    meta = _h2d(torch.tensor([offsets, lengths], dtype=torch.int64), dev)
    out = torch.empty(len(flat), 1, target, device=dev, dtype=torch.float32)
    K.LIB("mer_wav_pad_crop", len(flat), target, packed.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(),
          out.data_ptr(), K.stream_ptr())
    return out


def waveform_windows(wav: torch.Tensor, starts, lengths, target: int, device=None) -> torch.Tensor:
    """Windows of ONE recording: mono waveform ``wav`` (fp32, host or device) -> ``[Nw, 1, target]`` on the GPU, row
    ``w`` = ``wav[starts[w] : starts[w] + lengths[w]]`` zero-padded at the end to ``target`` (``lengths[w] <= target``).
    Windows may overlap: they are offsets into the one buffer, which crosses PCIe once (plus one copy of the
    offsets / lengths), through the pad / crop kernel of ``pad_crop_waveforms``."""
    flat = wav.reshape(-1)
    if flat.dtype != torch.float32:
        raise ValueError("waveform_windows takes an fp32 waveform")
    dev = torch.device(device) if device is not None else (flat.device if flat.is_cuda else None)
    if dev is None or dev.type != "cuda":
        raise RuntimeError("waveform_windows assembles the windows on the MI355X; pass device='cuda'")
    meta = torch.stack([torch.as_tensor(starts, dtype=torch.int64).reshape(-1).cpu(),
                        torch.as_tensor(lengths, dtype=torch.int64).reshape(-1).cpu()])
    target, n, Nw = int(target), int(flat.numel()), int(meta.shape[1])
    if target <= 0:
        raise ValueError(f"target must be positive, got {target}")
    if Nw and (int(meta.min()) < 0 or int(meta[1].max()) > target or int((meta[0] + meta[1]).max()) > n):
        raise ValueError(f"a window reaches outside the recording of {n} samples or is longer than target {target}")
    packed = flat.to(dev).contiguous() if flat.is_cuda else _h2d(flat.contiguous(), dev)
    if not n:
        packed = torch.zeros(1, device=dev)
    meta = _h2d(meta, dev)
    out = torch.empty(Nw, 1, target, device=dev, dtype=torch.float32)
    K.LIB("mer_wav_pad_crop", Nw, target, packed.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(), out.data_ptr(),
          K.stream_ptr())
    return out


def resample_ratio(sr_in: int, sr_out: int = 16000):
    """``(up, down)``: ``sr_out / sr_in`` in lowest terms."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in <= 0 or sr_out <= 0:
        raise ValueError(f"sample rates must be positive, got {sr_in} -> {sr_out}")
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def resample_emitted(n_in: int, up: int, down: int) -> int:
    """Outputs a stream of ``n_in`` inputs has emitted (``ResampleStream``): every output whose newest input
    ``floor((o * down + half) / up)`` has arrived, ``half = 10 * max(up, down)``; equal rates copy."""
    if up == 1 and down == 1:
        return int(n_in)
    a = int(n_in) * up - 10 * max(up, down) - 1
    return 0 if a < 0 else a // down + 1


def polyphase_table(up: int, down: int) -> torch.Tensor:
    """fp32 ``[up, kmax]``, ``kmax = 2 * half // up + 1``: scipy ``resample_poly``'s filter by phase.  ``g =
    firwin(2 * half + 1, 1 / max(up, down), window=("kaiser", 5.0)) * up`` in fp64 (windowed sinc, normalised to unit
    sum), rounded to fp32 once; ``table[p, t] = g[p + t * up]``, 0 past the filter's end."""
    import numpy as np

    up, down = int(up), int(down)
    max_rate = max(up, down)
    half = 10 * max_rate
    n = 2 * half + 1
    m = np.arange(n, dtype=np.float64) - half
    cutoff = 1.0 / max_rate
    h = cutoff * np.sinc(cutoff * m) * np.kaiser(n, 5.0)
    g = h / h.sum() * up
    kmax = 2 * half // up + 1
    tab = np.zeros(up * kmax, dtype=np.float64)
    k = np.arange(n)
    tab[(k % up) * kmax + k // up] = g
    return torch.from_numpy(tab.astype(np.float32)).view(up, kmax)


class ResampleCount:
    """The two counts of a resampled stream on the host: inputs consumed and outputs emitted.  They follow from the
    chunk lengths alone, so one object serves as the only host mirror of the device counts: a ``ResampleStream``
    advances it at every push, and the streaming session's control plane reads (or, where no audio is resampled,
    advances) the same object."""

    def __init__(self, sr_in: int, sr_out: int = 16000):
        self.up, self.down = resample_ratio(sr_in, sr_out)
        self.sr_in, self.n_in, self.n_out = int(sr_in), 0, 0

    def advance(self, n: int) -> int:
        """``n`` more inputs; returns how many outputs they emit."""
        self.n_in += int(n)
        emitted = resample_emitted(self.n_in, self.up, self.down) - self.n_out
        self.n_out += emitted
        return emitted


_POLYPHASE = {}
RESAMPLE_MAX_SPAN = 12288  # floats of LDS one workgroup of the resampler may stage (csrc/stream.hip)


class ResampleStream:
    """A stream resampled ONCE, chunk by chunk, into a device ring (mer_resample_stream): ``sr_in`` -> ``sr_out``
    with scipy ``resample_poly``'s filter, bit-identical however the stream is cut into chunks.  Nothing is
    synthesised at the live edge: an output waits for the chunk that brings its newest input, a latency of
    ``10 * max(up, down) / up`` input samples.

    Device state: ``hist`` fp32 ``[2, kmax]`` (the last ``kmax`` inputs, double-buffered: a push reads one half and
    writes the other), ``counts`` int64 ``[2]`` (inputs consumed, outputs emitted); ``count`` (a ``ResampleCount``,
    the caller's when given) mirrors the two on the host, so no push reads the device back.  Output ``q`` lands in
    ``ring[q % cap]``.  All pushes of one stream must be issued on one HIP stream."""

    def __init__(self, sr_in: int, ring: torch.Tensor, sr_out: int = 16000, count: "ResampleCount" = None):
        if not ring.is_cuda:
            raise RuntimeError("ResampleStream runs on the MI355X kernels; keep the ring on the GPU")
        if ring.dtype != torch.float32 or ring.dim() != 1 or not ring.is_contiguous() or ring.numel() < 1:
            raise ValueError("the audio ring must be a contiguous fp32 [cap] tensor")
        self.up, self.down = resample_ratio(sr_in, sr_out)
        self.count = count if count is not None else ResampleCount(sr_in, sr_out)
        if (self.count.up, self.count.down) != (self.up, self.down):
            raise ValueError(f"the count given is for another rate than {sr_in} -> {sr_out}")
        self.sr_in, self.ring, self.cap = int(sr_in), ring, int(ring.numel())
        self.copy = self.up == 1 and self.down == 1
        self.kmax = 0 if self.copy else 2 * 10 * max(self.up, self.down) // self.up + 1
        if not self.copy and 255 * self.down // self.up + 1 + self.kmax > RESAMPLE_MAX_SPAN:
            raise ValueError(f"sample rate {sr_in}: the resampler stages at most {RESAMPLE_MAX_SPAN} inputs per block")
        dev = ring.device
        self.table = None
        if not self.copy:
            key = (dev, self.up, self.down)
            self.table = _POLYPHASE.get(key)
            if self.table is None:
                self.table = _POLYPHASE[key] = polyphase_table(self.up, self.down).to(dev)
        self._hist = torch.zeros(2, max(self.kmax, 1), device=dev, dtype=torch.float32)
        self.counts = torch.zeros(2, device=dev, dtype=torch.int64)
        self._cur = 0

    @property
    def n_in(self) -> int:
        return self.count.n_in

    @property
    def n_out(self) -> int:
        return self.count.n_out

    @property
    def hist(self) -> torch.Tensor:
        """The last ``kmax`` inputs (zeros before the stream start), oldest first."""
        return self._hist[self._cur, :self.kmax]

    def push(self, chunk: torch.Tensor) -> int:
        """Feed the next inputs (1-D fp32, host or device); returns how many outputs this chunk emitted."""
        flat = chunk.reshape(-1)
        if flat.dtype != torch.float32:
            raise ValueError("ResampleStream.push takes fp32 samples")
        n = int(flat.numel())
        if n == 0:
            return 0
        dev = self.ring.device
        flat = flat.to(dev).contiguous() if flat.is_cuda else _h2d(flat.contiguous(), dev)
        new = 1 - self._cur
        K.LIB("mer_resample_stream", self.up, self.down, self.kmax, None if self.copy else self.table.data_ptr(),
              flat.data_ptr(), n, self.n_in, None if self.copy else self._hist[self._cur].data_ptr(),
              None if self.copy else self._hist[new].data_ptr(), self.kmax, self.ring.data_ptr(), self.cap,
              self.counts.data_ptr(), K.stream_ptr())
        self._cur = new
        return self.count.advance(n)


def resample_plan(sr_in: int, sr_out: int):
    """``(up, down, kmax)`` of a whole-clip resample, refused on the host when a workgroup's input span would not fit
    the resampler's LDS limit (``kmax`` is 0 for equal rates: a copy)."""
    up, down = resample_ratio(sr_in, sr_out)
    if up == 1 and down == 1:
        return up, down, 0
    kmax = 2 * 10 * max(up, down) // up + 1
    if 255 * down // up + 1 + kmax > RESAMPLE_MAX_SPAN:
        raise ValueError(f"sample rate {sr_in}: the resampler stages at most {RESAMPLE_MAX_SPAN} inputs per block")
    return up, down, kmax


def _polyphase(dev, up: int, down: int) -> torch.Tensor:
    key = (dev, up, down)
    t = _POLYPHASE.get(key)
    if t is None:
        t = _POLYPHASE[key] = polyphase_table(up, down).to(dev)
    return t


def resample_outputs(n_in: int, up: int, down: int) -> int:
    """``ceil(n_in * up / down)``: the outputs of a whole clip of ``n_in`` samples (scipy ``resample_poly``)."""
    return -(-int(n_in) * int(up) // int(down))


def resample_needed_inputs(target: int, up: int, down: int) -> int:
    """How many leading input samples the first ``target`` outputs of a resampled clip read: output ``target - 1``
    has newest input ``floor(((target - 1) * down + half) / up)``, ``half = 10 * max(up, down)``, so one more than
    that.  A clip sliced to this length gives the same first ``target`` outputs as the whole clip."""
    target, up, down = int(target), int(up), int(down)
    if target <= 0:
        return 0
    if up == 1 and down == 1:
        return target
    return ((target - 1) * down + 10 * max(up, down)) // up + 1


def _pack_clips(wavs, dev):
    """Ragged 1-D fp32 clips -> (packed device buffer, host offsets, host lengths)."""
    flat = [w.reshape(-1) for w in wavs]
    for w in flat:
        if w.dtype != torch.float32:
            raise ValueError("waveforms must be fp32")
    lengths = [int(w.numel()) for w in flat]
    offsets = [0]
    for n in lengths[:-1]:
        offsets.append(offsets[-1] + n)
    if not sum(lengths):
        packed = torch.zeros(1, device=dev)
    elif all(not w.is_cuda for w in flat):  # gathered straight into ONE pinned host buffer (one pass), one H2D copy
        stage = torch.empty(sum(lengths), dtype=torch.float32, pin_memory=True)
        torch.cat(flat, out=stage)
        packed = stage.to(dev, non_blocking=True)  # the caching host allocator keeps the block until the copy ran
    else:
        packed = torch.cat([w.to(dev) if w.is_cuda else _h2d(w.contiguous(), dev) for w in flat])
    return packed, offsets, lengths


def resample_clips(wavs, sample_rate_in: int, sample_rate_out: int = 16000, target: int = None, device=None,
                   out: torch.Tensor = None) -> torch.Tensor:
    """Whole clips resampled on the GPU, ``sample_rate_in`` -> ``sample_rate_out``, zero-padded at the end or cropped
    to ``target`` outputs each: ``[B, target]`` fp32 (mer_resample_clips, one launch for the batch).

    ``wavs``: a ragged list of 1-D fp32 clips, or one tensor (1-D: one clip; 2-D: one clip per row), host or device,
    all at ``sample_rate_in``.  The filter is scipy ``resample_poly``'s (``polyphase_table``), a clip is zero outside
    its own samples, and every output has the bits ``ResampleStream`` gives for the same clip.  ``target=None`` keeps
    each clip's own ``ceil(len * up / down)`` outputs, so it takes one clip or clips of equal output count.  Outputs
    past ``target`` are never computed; ``resample_needed_inputs`` says how much of a clip they read.  ``out``: a
    contiguous fp32 ``[B, target]`` device tensor to write into.  Rates are refused (``ValueError``) before any
    device work when not positive or when a block's input span exceeds the resampler's LDS limit."""
    up, down, kmax = resample_plan(sample_rate_in, sample_rate_out)
    if isinstance(wavs, torch.Tensor):
        if wavs.dim() not in (1, 2):
            raise ValueError("resample_clips takes a list of 1-D clips or one 1-D / 2-D tensor")
        wavs = [wavs] if wavs.dim() == 1 else list(wavs.unbind(0))
    wavs = list(wavs)
    if not wavs:
        raise ValueError("empty waveform batch")
    dev = torch.device(device) if device is not None else next((w.device for w in wavs if w.is_cuda), None)
    if dev is None or dev.type != "cuda":
        raise RuntimeError("resample_clips runs on the MI355X kernels; pass device='cuda'")
    if target is None:
        nouts = {resample_outputs(w.numel(), up, down) for w in wavs}
        if len(nouts) != 1:
            raise ValueError("target=None takes one clip or clips of equal output count; pass target")
        target = nouts.pop()
    packed, offsets, lengths = _pack_clips(wavs, dev)
    return resample_packed(packed, offsets, lengths, sample_rate_in, sample_rate_out, target, out=out)


def resample_packed(packed: torch.Tensor, offsets, lengths, sample_rate_in: int, sample_rate_out: int, target: int,
                    out: torch.Tensor = None) -> torch.Tensor:
    """``resample_clips`` on clips that already lie in one device buffer: clip ``b`` is ``packed[offsets[b] :
    offsets[b] + lengths[b]]`` (host sequences; gaps between the clips, any alignment and overlaps are allowed --
    nothing outside a clip's own samples is read).  Every (offset, length) is checked against the buffer on the host
    (``ValueError``) before anything is launched."""
    up, down, kmax = resample_plan(sample_rate_in, sample_rate_out)
    if not packed.is_cuda:
        raise RuntimeError("resample_packed runs on the MI355X kernels; move the packed clips to the GPU")
    if packed.dtype != torch.float32 or packed.dim() != 1 or not packed.is_contiguous():
        raise ValueError("packed must be a contiguous 1-D fp32 tensor")
    offsets, lengths = [int(o) for o in offsets], [int(n) for n in lengths]
    B, target, dev = len(offsets), int(target), packed.device
    if len(lengths) != B or not B:
        raise ValueError(f"{B} offsets for {len(lengths)} lengths")
    if target < 0 or B > 65535:
        raise ValueError(f"target {target} must not be negative, and at most 65535 clips go in one launch (got {B})")
    for o, n in zip(offsets, lengths):
        if o < 0 or n < 0 or o + n > int(packed.numel()):
            raise ValueError(f"clip [{o}, {o + n}) reaches outside the packed buffer of {int(packed.numel())} samples")
    if out is None:
        out = torch.empty(B, target, device=dev, dtype=torch.float32)
    elif tuple(out.shape) != (B, target) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"the resampler's out must be contiguous fp32 [{B}, {target}] on {dev}")
    if target:
        meta = _h2d(torch.tensor([offsets, lengths], dtype=torch.int64), dev)
        K.LIB("mer_resample_clips", B, target, up, down, kmax, _polyphase(dev, up, down).data_ptr() if kmax else None,
              packed.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(), out.data_ptr(), K.stream_ptr())
    return out


AUDIO_SNRS_DB = (20.0, 15.0, 10.0)  # ravdess.py:533, the SNRs drawn at level in [0.5, 0.9); 5 dB above


def draw_audio_augment(rng, target: int, n_noise: int) -> tuple:
    """One clip's audio draws of ravdess.py:519-576 from a numpy Generator, in ``load_audio_wav``'s order:
    ``uniform`` (the level), then ``choice`` of the SNR when ``0.5 <= level < 0.9`` (5 dB above, nothing below 0.5),
    then ``integers`` for the start in the bar-noise track of ``n_noise`` samples (tiled when shorter than ``target``)
    when ``max_start > 0``.  Returns ``(mode, start, snr_db, seed)`` for ``mix_noise_clips``: mode 0 leaves the clip
    alone, 1 mixes the track in, 2 (``n_noise == 0``) is the Gaussian fallback, whose one draw is a 63-bit seed in
    place of the host's ``rng.normal`` (the audio draws are an item's last, so nothing downstream shifts)."""
    target, n = int(target), int(n_noise)
    level = rng.uniform(0.0, 1.0)
    if level < 0.5:
        return 0, 0, 0.0, 0
    snr_db = float(rng.choice(list(AUDIO_SNRS_DB))) if level < 0.9 else 5.0
    if n > 0:
        tiled = n if n >= target else n * (target // n + 1)
        max_start = max(0, tiled - target)
        start = int(rng.integers(0, max_start + 1)) if max_start > 0 else 0
        return 1, start, snr_db, 0
    return 2, 0, snr_db, int(rng.integers(0, 2 ** 63 - 1))


def mix_noise_clips(wav: torch.Tensor, params: Sequence[tuple], bar_noise: torch.Tensor = None,
                    return_scale: bool = False):
    """The train-split noise mix (ravdess.py:539-576) of a waveform batch on the GPU: ``wav`` fp32 ``[B, target]`` or
    ``[B, 1, target]`` + one ``draw_audio_augment`` tuple ``(mode, start, snr_db, seed)`` per clip -> a new tensor
    of the same shape (mer_mix_noise_clips).

    Mode 1: ``clip(wav + noise[(start + i) % n] * scale, -1, 1)`` with ``scale = sqrt(ps / max(10^(snr/10), 1e-8) /
    pn)`` from the fp64 mean powers of the row and of the noise window (1 when ``pn <= 1e-8``), the host
    ``data.mix_noise``'s rule.  Mode 2: Gaussian noise of that target power from the augmentation's hashed
    ``normal_table`` draw per (seed, sample).  Mode 0: copied bit for bit, not clamped.  ``bar_noise``: the 16 kHz
    track, 1-D fp32 on the device (``ClipLoader`` uploads it once).  The descriptors are validated here before any
    launch.  ``return_scale=True`` also returns the ``[B]`` fp32 factors the device used (mode 2: sigma; mode 0: 0)."""
    if wav.dtype != torch.float32 or wav.dim() not in (2, 3) or (wav.dim() == 3 and wav.shape[1] != 1):
        raise ValueError("wav must be fp32 [B, target] or [B, 1, target]")
    B, target = int(wav.shape[0]), int(wav.shape[-1])
    if len(params) != B:
        raise ValueError(f"{len(params)} augmentation draws for {B} clips")
    dev = wav.device
    n_noise = 0
    if bar_noise is not None:
        if bar_noise.dtype != torch.float32 or bar_noise.dim() != 1 or bar_noise.device != dev:
            raise ValueError(f"bar_noise must be a 1-D fp32 tensor on {dev}")
        bar_noise = bar_noise.contiguous()
        n_noise = int(bar_noise.numel())
    for mode, start, snr_db, seed in params:
        if mode not in (0, 1, 2):
            raise ValueError(f"audio augmentation mode {mode!r}: 0 (none), 1 (noise track) or 2 (Gaussian)")
        if mode == 1 and not n_noise:
            raise ValueError("a mode-1 clip needs the bar-noise track")
        if not 0 <= int(start) < 2 ** 62 or not 0 <= int(seed) < 2 ** 63 or not math.isfinite(float(snr_db)):
            raise ValueError(f"bad audio augmentation draw (start {start}, snr_db {snr_db}, seed {seed})")
    if not wav.is_cuda:
        raise RuntimeError("mix_noise_clips runs on the MI355X kernels; move the waveforms to the GPU")
    src = wav.contiguous()
    out = torch.empty_like(src)
    scale = torch.empty(B, device=dev, dtype=torch.float32)
    if B and target:
        ints = _h2d(torch.tensor([[int(m), int(s), int(sd)] for m, s, _, sd in params], dtype=torch.int64).t()
                    .contiguous(), dev)
        modes = ints[0].to(torch.int32)
        snrs = _h2d(torch.tensor([float(s) for _, _, s, _ in params], dtype=torch.float32), dev)
        parts = torch.empty(B, -(-target // 256), 2, device=dev, dtype=torch.float64)
        K.LIB("mer_mix_noise_clips", B, target, src.data_ptr(), modes.data_ptr(), ints[1].data_ptr(), snrs.data_ptr(),
              ints[2].data_ptr(), bar_noise.data_ptr() if n_noise else None, n_noise, _ztable(dev).data_ptr(),
              parts.data_ptr(), scale.data_ptr(), out.data_ptr(), K.stream_ptr())
    return (out, scale) if return_scale else out


def assemble_waveforms(wavs: Sequence[torch.Tensor], sample_rates: Sequence[int], params: Sequence[tuple] = None,
                       bar_noise: torch.Tensor = None, sample_rate: int = 16000, duration_sec: float = 3.0,
                       device=None) -> torch.Tensor:
    """``load_audio_wav`` after the decode, for a batch, on the GPU: decoded mono clips at their native rates ->
    ``[B, 1, int(sample_rate * duration_sec)]``.  The batch is grouped by input rate: clips already at
    ``sample_rate`` take the pad / crop kernel of ``pad_crop_waveforms``, every other rate one ``resample_clips``
    launch; the rows land in batch order.  ``params`` (one ``draw_audio_augment`` tuple per clip, or None) then goes
    through ``mix_noise_clips`` with the device track ``bar_noise``; with no clip to augment the mix is skipped.
    Clips may be pre-sliced to ``resample_needed_inputs`` samples: the result is the same."""
    wavs = list(wavs)
    if not wavs:
        raise ValueError("empty waveform batch")
    if len(sample_rates) != len(wavs):
        raise ValueError(f"{len(sample_rates)} sample rates for {len(wavs)} clips")
    sr_out, target = int(sample_rate), int(sample_rate * duration_sec)
    groups = {}
    for i, sr in enumerate(sample_rates):
        groups.setdefault(int(sr), []).append(i)
    for sr in groups:
        resample_plan(sr, sr_out)  # every refusal before any device work
    dev = torch.device(device) if device is not None else next((w.device for w in wavs if w.is_cuda), None)
    if dev is None or dev.type != "cuda":
        raise RuntimeError("assemble_waveforms assembles the batch on the MI355X; pass device='cuda'")
    if len(groups) == 1:
        sr = next(iter(groups))
        audio = pad_crop_waveforms(wavs, sr_out, duration_sec, device=dev) if sr == sr_out else \
            resample_clips(wavs, sr, sr_out, target, device=dev).unsqueeze(1)
    else:
        audio = torch.empty(len(wavs), 1, target, device=dev, dtype=torch.float32)
        for sr, idx in groups.items():
            sub = [wavs[i] for i in idx]
            rows = pad_crop_waveforms(sub, sr_out, duration_sec, device=dev)[:, 0] if sr == sr_out else \
                resample_clips(sub, sr, sr_out, target, device=dev)
            K.rows_scatter(rows, idx, audio.view(len(wavs), target))
    if params is not None and any(p[0] for p in params):
        audio = mix_noise_clips(audio, params, bar_noise)
    return audio


MEL_N_FFT, MEL_HOP, MEL_BINS, MEL_BINS_PAD = 400, 160, 201, 208


def mel_tables(n_mels: int = 64, sample_rate: int = 16000):
    """Host tables of ``log_mel`` (fp64, rounded to fp32 once): ``(ctab, stab, fb)``.

    ``ctab`` / ``stab`` ``[400][208]``: the periodic Hann window times cos / sin(2 pi n f / 400), so the windowed DFT
    is one matrix product on the raw frame; ``fb`` ``[208][n_mels rounded up to 16]``: the HTK mel filterbank of
    ``torchaudio.functional.melscale_fbanks(201, 0, sr / 2, n_mels, sr, norm=None)``.  Padding columns / rows are 0."""
    n = torch.arange(MEL_N_FFT, dtype=torch.float64)
    win = 0.5 - 0.5 * torch.cos(2.0 * math.pi * n / MEL_N_FFT)  # torch.hann_window(400, periodic=True)
    # n * f mod 400 keeps the angle in [0, 2 pi): exact integer arithmetic before the one multiplication
    nf = torch.remainder(n[:, None] * torch.arange(MEL_BINS, dtype=torch.float64)[None, :], MEL_N_FFT)
    ang = 2.0 * math.pi * nf / MEL_N_FFT
    ctab = torch.zeros(MEL_N_FFT, MEL_BINS_PAD, dtype=torch.float64)
    stab = torch.zeros_like(ctab)
    ctab[:, :MEL_BINS] = win[:, None] * torch.cos(ang)
    stab[:, :MEL_BINS] = win[:, None] * torch.sin(ang)
    all_freqs = torch.linspace(0, sample_rate // 2, MEL_BINS, dtype=torch.float64)
    m_max = 2595.0 * math.log10(1.0 + (sample_rate / 2.0) / 700.0)
    m_pts = torch.linspace(0.0, m_max, n_mels + 2, dtype=torch.float64)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    down, up = -slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]
    fb = torch.zeros(MEL_BINS_PAD, -(-n_mels // 16) * 16, dtype=torch.float64)
    fb[:MEL_BINS, :n_mels] = torch.clamp(torch.minimum(down, up), min=0.0)
    return ctab.float().contiguous(), stab.float().contiguous(), fb.float().contiguous()


_MEL_TABLES = {}


def log_mel(wav: torch.Tensor, n_mels: int = 64, sample_rate: int = 16000, n_fft: int = 400, win_length: int = 400,
            hop_length: int = 160, to_db: bool = True) -> torch.Tensor:
    """Waveforms ``[B, 1, S]`` or ``[B, S]`` fp32 on the GPU -> ``[B, 1, n_mels, 1 + S // 160]`` fp32: the mel power
    spectrogram in dB (``10 log10(max(mel, 1e-10))``), or the power itself with ``to_db=False``.  Periodic Hann
    window, ``center=True`` with reflect padding, power 2, HTK mel scale from 0 to ``sample_rate / 2``, no
    normalisation -- the transform of ravdess.py:478-485, whose only free parameter is ``n_mels``."""
    if win_length != n_fft:
        raise ValueError(f"log_mel: win_length {win_length} != n_fft {n_fft} is not built (the reference never uses it)")
    if n_fft != MEL_N_FFT or hop_length != MEL_HOP:
        raise ValueError("log_mel is built for n_fft = win_length = 400, hop_length = 160 (ravdess.py:478-483)")
    if not 1 <= int(n_mels) <= 128:
        raise ValueError(f"log_mel: n_mels {n_mels} outside 1..128")
    if wav.dim() == 3 and wav.shape[1] == 1:
        wav = wav[:, 0]
    if wav.dim() != 2 or wav.dtype != torch.float32:
        raise ValueError("log_mel takes fp32 waveforms [B, 1, S] or [B, S]")
    B, S = wav.shape
    if S <= n_fft // 2:
        raise ValueError(f"log_mel: reflect padding of {n_fft // 2} samples needs more than {n_fft // 2} samples, got {S}")
    if not wav.is_cuda:
        raise RuntimeError("log_mel runs on the MI355X kernels; move the waveforms to the GPU")
    if wav.stride(1) != 1 or wav.stride(0) < S:
        wav = wav.contiguous()
    key = (wav.device, int(n_mels), int(sample_rate))
    tabs = _MEL_TABLES.get(key)
    if tabs is None:
        tabs = _MEL_TABLES[key] = tuple(t.to(wav.device) for t in mel_tables(int(n_mels), int(sample_rate)))
    T = 1 + S // MEL_HOP
    out = torch.empty(B, 1, int(n_mels), T, device=wav.device, dtype=torch.float32)
    if B:
        K.LIB("mer_log_mel", B, S, int(n_mels), wav.data_ptr(), wav.stride(0), tabs[0].data_ptr(), tabs[1].data_ptr(),
              tabs[2].data_ptr(), int(bool(to_db)), out.data_ptr(), K.stream_ptr())
    return out
