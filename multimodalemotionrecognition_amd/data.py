"""Real input pipeline: ``src/data/ravdess.py``'s clip loading with the host work in native
code (``host/mer_io.cpp`` -> ``libmer_io.so``, C-ABI ``include/mer_io.h``) and the batch assembly on the MI355X
(``clips.py`` -> ``csrc/clips.hip``).

* ``load_audio_wav`` -- ravdess.py:488-578: WAV decode + mono mix + resample to 16 kHz (native), pad / crop to
  3 s, bar-noise augmentation at a drawn SNR (native mix).  librosa's soxr_hq resampler is absent from this image:
  the native resampler restates ``scipy.signal.resample_poly`` (parity with soxr unpinned; pinned against scipy).
* ``uniform_indices`` -- ravdess.py:272-277, the frame sampling of ``load_video_frames``.
* ``face_crop_box`` -- face_crop.py:151-190 (``crop_with_padding``'s box, pad 0.3).
* ``load_video_frames`` -- ravdess.py:280-390 after decode: index sampling, face-box crop, resize + /255 +
  ImageNet normalisation on the device.  Video DECODING (cv2.VideoCapture) and face DETECTION (MediaPipe) need
  libraries this image does not have: the caller supplies decoded RGB uint8 frames (any decoder) and, optionally,
  the detected bbox; without one the full frame is used -- the reference's own fallback when MediaPipe is missing
  (ravdess.py:300-304).
* ``ClipLoader`` -- the DataLoader of train.py for the GPU path: worker threads decode clips (the native calls
  release the GIL), each rank takes a disjoint shard (DP), and batches land in HBM as
  ``[B, 8, 3, 112, 112]`` / ``[B, 1, 48000]`` / labels.  ``device_audio=True`` leaves only the WAV decode and the
  draws to the workers: resampling, pad / crop and the noise mix run on the device (``clips.assemble_waveforms``).
  ``device_video=True`` packs a batch's cropped clips into one pinned buffer: one copy and one ragged resize launch
  per batch (``clips.crop_resize_frames``) instead of one of each per clip.
"""
from __future__ import annotations

import ctypes
import queue
import threading
from pathlib import Path
from typing import Callable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import clips

_LIB_PATH = Path(__file__).resolve().parent / "libmer_io.so"
_lib = None
_lock = threading.Lock()

IO_ERRORS = {-1: "cannot open / read the file", -2: "not a RIFF/WAVE file or unsupported sample format",
             -3: "bad argument"}


class MerIOError(RuntimeError):
    pass


def _io():
    global _lib
    with _lock:
        if _lib is None:
            if not _LIB_PATH.exists():
                raise MerIOError(f"host input library not built: {_LIB_PATH} is missing (make -C "
                                 "multimodalemotionrecognition_amd/host, or __graft_entry__.build())")
            lib = ctypes.CDLL(str(_LIB_PATH))
            P, I, LL, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
            sig = {
                "mer_wav_info": (I, [ctypes.c_char_p, P, P, P, P, P]),
                "mer_wav_read_mono": (I, [ctypes.c_char_p, P, LL, P]),
                "mer_resample_len": (LL, [LL, I, I]),
                "mer_resample": (I, [P, LL, I, I, P, LL, P]),
                "mer_uniform_indices": (I, [I, I, P]),
                "mer_face_crop_box": (I, [I, I, I, I, I, I, F, P]),
                "mer_mix_noise": (I, [P, LL, P, LL, LL, F]),
            }
            for name, (res, args) in sig.items():
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
            _lib = lib
    return _lib


def _check(rc, what):
    if rc != 0:
        raise MerIOError(f"{what}: {IO_ERRORS.get(rc, rc)}")


def wav_info(path) -> dict:
    sr, ch, fr, fmt, bits = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong(), ctypes.c_int(), ctypes.c_int()
    _check(_io().mer_wav_info(str(path).encode(), ctypes.byref(sr), ctypes.byref(ch), ctypes.byref(fr),
                              ctypes.byref(fmt), ctypes.byref(bits)), f"wav_info({path})")
    return {"sample_rate": sr.value, "channels": ch.value, "frames": fr.value, "format": fmt.value, "bits": bits.value}


def read_wav_mono(path) -> Tuple[np.ndarray, int]:
    """(float32 mono samples, native sample rate) -- soundfile scaling, channel mean (librosa.load with sr=None)."""
    info = wav_info(path)
    out = np.empty(max(1, info["frames"]), dtype=np.float32)
    n = ctypes.c_longlong()
    _check(_io().mer_wav_read_mono(str(path).encode(), out.ctypes.data, out.size, ctypes.byref(n)), f"read({path})")
    return out[:n.value], info["sample_rate"]


def resample(x: np.ndarray, sr_in: int, sr_out: int) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = _io().mer_resample_len(x.size, sr_in, sr_out)
    if n < 0:
        raise MerIOError("resample: bad rates")
    out = np.empty(max(1, n), dtype=np.float32)
    got = ctypes.c_longlong()
    _check(_io().mer_resample(x.ctypes.data, x.size, sr_in, sr_out, out.ctypes.data, out.size, ctypes.byref(got)),
           "resample")
    return out[:got.value]


def uniform_indices(total: int, num: int) -> List[int]:
    out = np.empty(max(1, num), dtype=np.int32)
    _check(_io().mer_uniform_indices(int(total), int(num), out.ctypes.data), "uniform_indices")
    return out[:num].tolist()


def face_crop_box(h: int, w: int, bbox, pad_ratio: float = 0.3) -> Tuple[int, int, int, int]:
    out = np.empty(4, dtype=np.int32)
    x1, y1, x2, y2 = (int(v) for v in bbox)
    _check(_io().mer_face_crop_box(int(h), int(w), x1, y1, x2, y2, float(pad_ratio), out.ctypes.data), "crop box")
    return tuple(int(v) for v in out)


def mix_noise(wav: np.ndarray, noise: np.ndarray, start: int, snr_db: float) -> np.ndarray:
    """In place on a float32 copy; returns it (ravdess.py:543-566)."""
    w = np.array(wav, dtype=np.float32, copy=True)
    nz = np.ascontiguousarray(noise, dtype=np.float32).reshape(-1)
    _check(_io().mer_mix_noise(w.ctypes.data, w.size, nz.ctypes.data, nz.size, int(start), float(snr_db)), "mix")
    return w


def load_audio_wav(audio_path, sample_rate: int = 16000, duration_sec: float = 3.0, augment: bool = False,
                   bar_noise: Optional[np.ndarray] = None, rng: Optional[np.random.Generator] = None) -> torch.Tensor:
    """ravdess.py:488-578 -> host float32 ``[1, int(sample_rate * duration_sec)]``.  ``bar_noise``: the 16 kHz bar
    noise track (the reference's ``_load_bar_noise``); without one, augmentation falls back to Gaussian noise at
    the drawn SNR as the reference does."""
    wav, sr = read_wav_mono(audio_path)
    if sr != sample_rate:
        wav = resample(wav, sr, sample_rate)
    target = int(sample_rate * duration_sec)
    if wav.size < target:
        wav = np.pad(wav, (0, target - wav.size))
    else:
        wav = wav[:target]
    if augment:
        rng = rng if rng is not None else np.random.default_rng()
        level = rng.uniform(0.0, 1.0)
        if level >= 0.5:
            snr_db = float(rng.choice([20.0, 15.0, 10.0])) if level < 0.9 else 5.0
            if bar_noise is not None and bar_noise.size:
                n = bar_noise.size
                tiled = n if n >= target else n * (target // n + 1)
                max_start = max(0, tiled - target)
                start = int(rng.integers(0, max_start + 1)) if max_start > 0 else 0
                wav = mix_noise(wav, bar_noise, start, snr_db)
            else:
                p = float(np.mean(wav.astype(np.float32) ** 2))
                noise = rng.normal(0, np.sqrt(p / max(10 ** (snr_db / 10.0), 1e-8)), wav.shape).astype(np.float32)
                wav = np.clip(wav + noise, -1.0, 1.0)
    return torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32)).unsqueeze(0)


FrameSource = Union[np.ndarray, torch.Tensor, Callable[[], np.ndarray], str, Path]


def _frames(src: FrameSource) -> np.ndarray:
    """Decoded RGB uint8 frames [T, H, W, 3]: an array, a ``.npy`` file or a decoder callable."""
    if callable(src):
        src = src()
    if isinstance(src, (str, Path)):
        src = np.load(str(src), allow_pickle=False)
    if isinstance(src, torch.Tensor):
        src = src.cpu().numpy()
    a = np.asarray(src)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[-1] != 3:
        raise ValueError("decoded frames must be uint8 [T, H, W, 3] RGB")
    return a


def select_frames(frames: np.ndarray, num_frames: int = 8, bbox=None, pad_ratio: float = 0.3) -> np.ndarray:
    """The host half of load_video_frames: uniform sampling, face-box crop (one box for every frame, as the
    reference reuses the first frame's detection), padding by repeating the last frame -> [num_frames, h, w, 3]."""
    T, H, W, _ = frames.shape
    if T == 0:
        return np.zeros((num_frames, 1, 1, 3), dtype=np.uint8)
    idx = [min(i, T - 1) for i in uniform_indices(T, num_frames)]
    sel = frames[idx]
    if bbox is not None:
        x1, y1, x2, y2 = face_crop_box(H, W, bbox, pad_ratio)
        if x2 > x1 and y2 > y1:
            sel = sel[:, y1:y2, x1:x2]
    return np.ascontiguousarray(sel)


def load_video_frames(src: FrameSource, num_frames: int = 8, size: int = 112, bbox=None,
                      device="cuda") -> torch.Tensor:
    """ravdess.py:280-390 after decode -> ``[num_frames, 3, size, size]`` fp32 on the device."""
    sel = select_frames(_frames(src), num_frames, bbox)
    dev_frames = torch.from_numpy(sel).to(device, non_blocking=False)
    return clips.preprocess_frames(dev_frames, size)


def _collate_meta(metas: List[dict]) -> dict:
    """default_collate of the reference's per-clip meta dicts (ravdess.py:608-615): one list per key (ints as a
    tensor, as torch's collate does)."""
    keys = []
    for m in metas:
        keys += [k for k in m if k not in keys]
    out = {}
    for k in keys:
        vals = [m.get(k) for m in metas]
        out[k] = torch.tensor(vals) if all(isinstance(v, int) and not isinstance(v, bool) for v in vals) else vals
    return out


def shard_indices(n: int, rank: int, world: int, shuffle: bool, seed: int, epoch: int,
                  pad: bool = True) -> np.ndarray:
    """``torch.utils.data.DistributedSampler`` order (drop_last=False): one permutation of ALL items drawn by
    ``torch.randperm`` from a CPU generator seeded with (seed + epoch) on every rank -- the sampler's own draw, so
    the shuffled order is the reference pipeline's --, padded by wrapping to a multiple of ``world``, then every
    ``world``-th index from ``rank``: every rank sees the same number of items and, across epochs, different clips.
    ``pad=False`` (evaluation: no clip counted twice): no wrapping, the ranks' shards partition the items exactly
    and may differ by one item."""
    if shuffle:
        order = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed) + int(epoch))).numpy()
    else:
        order = np.arange(n)
    if not pad:
        return order[rank:n:world]
    total = -(-n // world) * world if n else 0
    if total > n:
        reps = -(-(total - n) // n)
        order = np.concatenate([order] + [order] * reps)[:total]
    return order[rank:total:world]


class ClipLoader:
    """Batches of ``(video [B, 8, 3, 112, 112], audio [B, 1, 48000], labels [B], meta)`` assembled on the GPU --
    the 4-tuples of the reference's datasets (ravdess.py:616, 654) that ``train_one_epoch`` unpacks
    (train.py:200).

    ``items``: ``(frames source, wav path, label[, bbox-or-None[, meta dict]])`` per clip.  Data parallelism:
    rank ``rank`` of ``world`` takes a ``DistributedSampler``-style shard of one global permutation
    (``shard_indices``), so all ranks run the same number of steps (a rank with an extra step would block in the
    gradient all-reduce); ``pad_shards=False`` (evaluation) takes an exact partition instead, with no clip wrapped
    round to fill the last shard.  ``workers`` threads decode ahead (``prefetch`` batches).  ``augment``: the
    reference's train-split audio augmentation (ravdess.py:519-578, bar noise at a drawn SNR; ``bar_noise`` is the 16 kHz
    track, else Gaussian noise), drawn from a generator seeded per (seed, epoch, item) so the draws do not depend
    on thread scheduling.  ``augment`` also applies the reference's train-split video augmentation
    (cv2.GaussianBlur(k, 0) + darken + Gaussian noise on the uint8 frames, ravdess.py:366-384) on the device, one
    ``clips.augment_clips`` launch per batch with per-clip draws from the same generator; it is bit-exact against
    the restatement in ``oracle/clips_ref.py``, and parity against cv2 itself is unpinned (cv2 is absent here).
    ``audio_features="mel"``: ``audio`` is ``clips.log_mel`` of the waveform batch, ``[B, 1, n_mels, 301]`` (what the
    mel ``AudioNet`` models take); the default ``"wav"`` yields the waveforms.

    ``device_audio=True`` moves the audio work after the WAV decode to the GPU: a worker only decodes the file at its
    native rate, slices it to the samples the kept outputs read (``clips.resample_needed_inputs``) and makes the
    augmentation draws (``clips.draw_audio_augment``, the host's draws in the host's order); the batch then crosses
    PCIe as one packed pinned copy per input rate and ``clips.assemble_waveforms`` resamples, pads / crops and mixes
    the noise there (the track is uploaded once per loader).  Against the default it differs by the resampler's
    rounding (fp32 fmaf sums against the host's double-rounded taps) and, with no bar-noise track, by the Gaussian
    fallback's generator; video, labels and every draw are the same.  The default (``False``) is the host path.

    ``device_video=True`` batches the video side of the assembly.  The workers do what they always did (sample on the
    host and apply the face crop there, so only the crops cross PCIe, never whole frames); the producer thread then
    gathers the batch's crops, which differ in size, into ONE pinned buffer (``clips.stage_frames``), and ``_assemble``
    issues one asynchronous host-to-device copy and ONE ragged launch (``clips.crop_resize_frames``: fp32 for eval,
    uint8 feeding ``augment_clips`` for the train split) instead of one blocking pageable copy and one launch per
    clip.  Batches are bit-identical to the default; items, draw order and ``meta`` are unchanged."""

    def __init__(self, items: Sequence[Tuple], batch_size: int = 32, num_frames: int = 8, size: int = 112,
                 sample_rate: int = 16000, duration_sec: float = 3.0, rank: int = 0, world: int = 1,
                 workers: int = 8, prefetch: int = 2, device="cuda", shuffle: bool = False, seed: int = 0,
                 drop_last: bool = True, augment: bool = False, bar_noise: Optional[np.ndarray] = None,
                 pad_shards: bool = True, audio_features: str = "wav", n_mels: int = 64, device_audio: bool = False,
                 device_video: bool = False):
        self.all_items = list(items)
        if audio_features not in ("wav", "mel"):
            raise ValueError(f"audio_features must be 'wav' or 'mel', got {audio_features!r}")
        self.audio_features, self.n_mels = audio_features, int(n_mels)
        self.rank, self.world = int(rank), max(1, int(world))
        if not 0 <= self.rank < self.world:
            raise ValueError(f"rank {rank} outside world {world}")
        self.B, self.T, self.size = batch_size, num_frames, size
        self.sr, self.dur = sample_rate, duration_sec
        self.workers, self.prefetch = max(1, workers), max(1, prefetch)
        self.device = torch.device(device)
        self.shuffle, self.seed, self.drop_last = shuffle, seed, drop_last
        self.augment, self.bar_noise = bool(augment), bar_noise
        self.pad_shards = bool(pad_shards)
        self.device_audio = bool(device_audio)
        self._bar_dev = None  # the bar-noise track on the device, uploaded once (device_audio)
        self.device_video = bool(device_video)
        if self.device_audio and self.device.type != "cuda":
            raise RuntimeError("ClipLoader(device_audio=True) runs on the MI355X kernels; pass device='cuda'")
        if self.device_video and self.device.type != "cuda":
            raise RuntimeError("ClipLoader(device_video=True) runs on the MI355X kernels; pass device='cuda'")
        self.epoch = 0

    @property
    def items(self):
        """This rank's items in epoch-0 order."""
        return [self.all_items[i] for i in shard_indices(len(self.all_items), self.rank, self.world, False, 0, 0,
                                                           pad=self.pad_shards)]

    def num_samples(self) -> int:
        n = len(self.all_items)
        if not self.pad_shards:  # this rank's part of an exact partition
            return len(range(self.rank, n, self.world))
        return -(-n // self.world) if n else 0

    def __len__(self):
        n = self.num_samples()
        return n // self.B if self.drop_last else -(-n // self.B)

    def _stage_video(self, decoded):
        """``device_video``, host half (the producer thread): the batch's cropped clips, which differ in size, gathered
        into ONE pinned buffer, and the descriptor table of the ragged resize -- whole images: the workers cropped
        them."""
        stage, offsets = clips.stage_frames([d[0] for d in decoded])
        hw = np.array([d[0].shape[1:3] for d in decoded for _ in range(d[0].shape[0])], dtype=np.int64)
        rects = np.concatenate([np.zeros_like(hw), hw[:, ::-1]], axis=1)
        return stage, clips.crop_rows(offsets, hw[:, 0], hw[:, 1], rects)

    def _assemble_video(self, decoded, staged=None):
        """``device_video``, device half: one host-to-device copy of the pinned buffer and one ragged resize launch
        over all ``B * T`` frames (fp32 for eval, uint8 feeding ``augment_clips`` for the train split)."""
        stage, rows = staged if staged is not None else self._stage_video(decoded)
        buf = stage.to(self.device, non_blocking=True)  # the caching host allocator keeps the block until it ran
        B = len(decoded)
        if self.augment:
            u8 = clips.crop_resize_frames(buf, rows, self.size, u8=True)
            return clips.augment_clips(u8.view(B, self.T, self.size, self.size, 3), [d[4] for d in decoded])
        return clips.crop_resize_frames(buf, rows, self.size).view(B, self.T, 3, self.size, self.size)

    def _assemble(self, decoded, staged=None):
        # frames of one batch may differ in size (per-clip crops): resize each clip's frames on the device
        if self.device_video:
            video = self._assemble_video(decoded, staged)
        elif self.augment:  # resized uint8 clips, then ONE augmentation + normalisation launch with per-clip draws
            u8 = torch.empty(len(decoded), self.T, self.size, self.size, 3, device=self.device, dtype=torch.uint8)
            for i, d in enumerate(decoded):
                clips.resize_frames_u8(torch.from_numpy(d[0]).to(self.device), self.size, out=u8[i])
            video = clips.augment_clips(u8, [d[4] for d in decoded])
        else:
            vids = [clips.preprocess_frames(torch.from_numpy(d[0]).to(self.device), self.size) for d in decoded]
            video = torch.stack(vids).contiguous()
        wavs = [torch.from_numpy(d[1]) for d in decoded]
        if self.device_audio:  # native-rate clips: one packed pinned copy per rate, resample + pad / crop + mix there
            if self.augment and self._bar_dev is None and self.bar_noise is not None and self.bar_noise.size:
                track = np.ascontiguousarray(self.bar_noise, dtype=np.float32).reshape(-1)
                self._bar_dev = clips._h2d(torch.from_numpy(track), self.device)
            audio = clips.assemble_waveforms(wavs, [d[5][0] for d in decoded],
                                             [d[5][1] for d in decoded] if self.augment else None, self._bar_dev,
                                             self.sr, self.dur, device=self.device)
        else:
            audio = clips.pad_crop_waveforms(wavs, self.sr, self.dur, device=self.device)
        if self.audio_features == "mel":  # RavdessAVDataset's audio item (ravdess.py:607): [B, 1, n_mels, T]
            audio = clips.log_mel(audio, n_mels=self.n_mels, sample_rate=self.sr)
        labels = torch.tensor([d[2] for d in decoded], dtype=torch.long).to(self.device)
        return video, audio, labels, _collate_meta([d[3] for d in decoded])

    def __iter__(self):
        order = shard_indices(len(self.all_items), self.rank, self.world, self.shuffle, self.seed, self.epoch,
                              pad=self.pad_shards)
        epoch = self.epoch
        self.epoch += 1
        nb = len(self)
        batches = [order[i * self.B:(i + 1) * self.B] for i in range(nb)]
        out_q: "queue.Queue" = queue.Queue(maxsize=self.prefetch)
        stop = threading.Event()

        def produce():
            from concurrent.futures import ThreadPoolExecutor
            try:
                with ThreadPoolExecutor(self.workers) as ex:
                    for b in batches:
                        if stop.is_set():
                            return
                        decoded = list(ex.map(self._decode_epoch(epoch), [(int(i), self.all_items[i]) for i in b]))
                        staged = self._stage_video(decoded) if self.device_video else None
                        out_q.put(("ok", (decoded, staged)))
            except BaseException as e:  # surfaced to the consumer
                out_q.put(("err", e))
            out_q.put(("end", None))

        th = threading.Thread(target=produce, daemon=True)
        th.start()
        try:
            while True:
                kind, val = out_q.get()
                if kind == "end":
                    return
                if kind == "err":
                    raise val
                yield self._assemble(*val)
        finally:
            stop.set()

    def _decode_epoch(self, epoch):
        def fn(job):
            gi, item = job
            src, wav_path, label = item[0], item[1], item[2]
            bbox = item[3] if len(item) > 3 else None
            meta = dict(item[4]) if len(item) > 4 and item[4] is not None else {}
            meta.setdefault("index", int(gi))
            frames = select_frames(_frames(src), self.T, bbox)
            rng = np.random.default_rng([self.seed, epoch, int(gi)]) if self.augment else None
            # the reference loads (and augments) the video before the audio (ravdess.py:639-645): same draw order
            vaug = clips.draw_video_augment(rng) if self.augment else None
            if self.device_audio:  # decode at the native rate, keep what the kept outputs read, make the draws
                wav, sr = read_wav_mono(wav_path)
                target = int(self.sr * self.dur)
                up, down, _ = clips.resample_plan(sr, self.sr)
                wav = np.ascontiguousarray(wav[:clips.resample_needed_inputs(target, up, down)])
                n_noise = int(self.bar_noise.size) if self.bar_noise is not None else 0
                aaug = clips.draw_audio_augment(rng, target, n_noise) if self.augment else None
                return frames, wav, int(label), meta, vaug, (int(sr), aaug)
            wav = load_audio_wav(wav_path, self.sr, self.dur, augment=self.augment, bar_noise=self.bar_noise,
                                 rng=rng)[0].numpy()
            return frames, wav, int(label), meta, vaug
        return fn
