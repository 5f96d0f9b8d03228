"""Time the device audio clip assembly with HIP events (5 warm-up runs, the median of 20, one process): B = 32 and 64
clips of 4 s at 48 kHz, half of them augmented -- (a) ``clips.resample_clips`` to 48,000 samples, (b)
``clips.mix_noise_clips``, (c) the pinned H2D copy of the sliced input -- beside the same clips through the host
functions (``data.resample`` + pad / crop + ``data.mix_noise``) in a ``ThreadPoolExecutor(8)``, which is what
``ClipLoader`` does today; then ``ClipLoader`` batches/s end to end over synthetic WAV files and 8 small frames per
clip, ``device_audio`` off and on.  Writes profiles/clips/bench_audio_assembly.json and prints it.
    python tools/bench_audio_assembly.py"""
import json
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from multimodalemotionrecognition_amd import clips  # noqa: E402
from multimodalemotionrecognition_amd import data as D  # noqa: E402
from oracle.io_ref import write_wav  # noqa: E402

WARMUP, RUNS = 5, 20
SR_IN, SR, SECONDS, TARGET = 48000, 16000, 4.0, 48000
STEP_MS = 4.65  # the train step of the README (B = 32)


def timed_ms(fn):
    """Median device time of one call, each run bracketed by its own pair of HIP events."""
    for _ in range(WARMUP):
        fn()
    ts = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def wall_ms(fn):
    for _ in range(WARMUP):
        fn()
    ts = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def assembly(B, bar):
    dev = "cuda"
    rng = np.random.default_rng(B)
    n_in = int(SR_IN * SECONDS)
    up, down = clips.resample_ratio(SR_IN, SR)
    need = clips.resample_needed_inputs(TARGET, up, down)
    wavs = [rng.normal(0, 0.1, n_in).astype(np.float32) for _ in range(B)]
    params = [(1, int(rng.integers(0, bar.size - TARGET)), float(rng.choice([20.0, 15.0, 10.0, 5.0])), 0) if b % 2
              else (0, 0, 0.0, 0) for b in range(B)]
    sliced = torch.cat([torch.from_numpy(w[:need]) for w in wavs]).pin_memory()
    offsets, lengths = [b * need for b in range(B)], [need] * B
    bar_dev = torch.from_numpy(bar).to(dev)
    packed = sliced.to(dev)
    out = torch.empty(B, TARGET, device=dev)
    res = {"B": B, "input_samples_per_clip": n_in, "sliced_samples_per_clip": need,
           "h2d_mbytes": round(sliced.numel() * 4 / 1e6, 2), "h2d_mbytes_at_16khz": round(B * TARGET * 4 / 1e6, 2)}
    a = timed_ms(lambda: clips.resample_packed(packed, offsets, lengths, SR_IN, SR, TARGET, out=out))
    b = timed_ms(lambda: clips.mix_noise_clips(out, params, bar_dev))
    c = timed_ms(lambda: sliced.to(dev, non_blocking=True))
    whole = timed_ms(lambda: clips.mix_noise_clips(
        clips.resample_packed(sliced.to(dev, non_blocking=True), offsets, lengths, SR_IN, SR, TARGET), params, bar_dev))
    res["device"] = {"resample_crop_ms": round(a, 4), "mix_ms": round(b, 4), "h2d_ms": round(c, 4),
                     "h2d_gbytes_per_s": round(sliced.numel() * 4 / c / 1e6, 1), "copy_resample_mix_ms": round(whole, 4),
                     "clips_per_s": round(B / whole * 1e3, 1)}

    def host_clip(job):
        w, p = job
        y = D.resample(w, SR_IN, SR)
        y = np.pad(y, (0, TARGET - y.size)) if y.size < TARGET else y[:TARGET]
        return D.mix_noise(y, bar, p[1], p[2]) if p[0] else y

    with ThreadPoolExecutor(8) as ex:
        h = wall_ms(lambda: list(ex.map(host_clip, zip(wavs, params))))
    res["host_8_threads"] = {"ms": round(h, 3), "clips_per_s": round(B / h * 1e3, 1)}
    res["device_over_host"] = round(h / whole, 1)
    res["device_share_of_train_step"] = round(whole / (STEP_MS * B / 32), 4)
    return res


def loader(tmp, bar, n_items=128, B=32):
    rng = np.random.default_rng(1)
    items = []
    for i in range(n_items):
        fp, wp = tmp / f"f{i}.npy", tmp / f"a{i}.wav"
        np.save(fp, rng.integers(0, 256, (8, 64, 64, 3), dtype=np.uint8))
        write_wav(wp, rng.normal(0, 0.1, int(SR_IN * SECONDS)).clip(-1, 1), SR_IN, "pcm16")
        items.append((str(fp), str(wp), i % 8))
    res = {"items": n_items, "B": B, "workers": 8, "frames": "8 x 64 x 64", "wav": "4 s, 48 kHz, PCM16"}
    for name, on in (("host_audio", False), ("device_audio", True)):
        ld = D.ClipLoader(items, batch_size=B, workers=8, augment=True, bar_noise=bar, device_audio=on)
        ts = []
        for _ in range(3):  # epochs; the first warms the file cache, the tables and the allocator
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = sum(1 for _ in ld)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        t = min(ts[1:])
        res[name] = {"batches_per_s": round(n / t, 2), "clips_per_s": round(n * B / t, 1)}
    res["device_over_host"] = round(res["device_audio"]["clips_per_s"] / res["host_audio"]["clips_per_s"], 2)
    return res


def main():
    bar = np.random.default_rng(0).uniform(-0.2, 0.2, 10 * SR).astype(np.float32)
    out = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "runs": RUNS, "train_step_ms": STEP_MS,
           "train_clips_per_s": round(32 / STEP_MS * 1e3), "assembly": [assembly(B, bar) for B in (32, 64)]}
    with tempfile.TemporaryDirectory() as tmp:
        out["clip_loader"] = loader(Path(tmp), bar)
    d = ROOT / "profiles" / "clips"
    d.mkdir(parents=True, exist_ok=True)
    (d / "bench_audio_assembly.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
