"""Live streaming sessions at the reference's defaults: N clients, each sending 6 fps of 112 x 112
frames and 48 kHz audio in 0.1 s chunks, 3 s windows, one prediction per client every 0.5 s -- xattn + WavLM +
ResNet18, random-init weights, host inputs (every frame and chunk crosses PCIe inside the timed region).

Two ways through the same M ticks, alternating tick by tick, each ending in a device synchronise:

* ``pool``: ``StreamingSessionPool`` -- the tick's frames and chunks go into the device rings (``add_frame`` /
  ``add_audio_chunk``), then one ``infer_ready`` for all sessions;
* ``clip_path``: the existing path doing the reference's work per client and tick -- the last 3 s of 48 kHz audio
  resampled on the host (``data.resample``: mer_resample), the window's frames picked by ``uniform_indices``,
  ``video_clip_batch`` on those 8 frames, ``predict_probs`` at batch 1.

Both start from buffers already holding 3 s (filled before the clock starts).  Prints one JSON line: median tick time
of each way, predictions per second, trunk frames per prediction, and the largest |dprob| between the two ways (not
zero: the pool resamples the stream once, the clip path each window with its own edge transients).
    python tools/bench_stream.py [--sessions 16] [--ticks 20] [--grid window|shared] [--stride 2]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from multimodalemotionrecognition_amd import clips, data  # noqa: E402
from multimodalemotionrecognition_amd.optimized_runtime import TorchModelRunner  # noqa: E402
from multimodalemotionrecognition_amd.train import build_model  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sessions", type=int, default=16)
ap.add_argument("--ticks", type=int, default=20)
ap.add_argument("--grid", default="window", choices=["window", "shared"])
ap.add_argument("--stride", type=int, default=2)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_stream measures on an MI355X: no GPU found")

FPS, SR_IN, WINDOW, STEP, T = 6, 48000, 3.0, 0.5, 8
CHUNK = SR_IN // 10
N, M = args.sessions, args.ticks
torch.manual_seed(0)
model = build_model(8, "xattn", pretrained_video=False, use_wavlm=True)
ck = {"model": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "val_f1": 0.0,
      "config": {"fusion": "xattn", "use_wavlm": True, "num_classes": 8}}
runner = TorchModelRunner(checkpoint=ck, device="cuda")
seconds = WINDOW + (M + 4) * STEP
g = torch.Generator().manual_seed(20261020)
n_frames = int(seconds * FPS) + 1
frames = [torch.randint(0, 256, (n_frames, 112, 112, 3), generator=g, dtype=torch.uint8).numpy() for _ in range(N)]
wavs = [((torch.rand(int(seconds * SR_IN), generator=g) - 0.5) * 0.5).numpy() for _ in range(N)]
pool = runner.open_stream_pool(N, frame_grid=args.grid, frame_stride=args.stride if args.grid == "shared" else None)
sessions = [pool.create_session() for _ in range(N)]
T0 = 1000.0
sent = dict(frames=0, chunks=0)


def feed(upto_sec):
    """Send every session what is stamped up to ``upto_sec`` and not sent yet; returns (frames, chunks) sent so far."""
    f1 = min(n_frames, int(np.floor(upto_sec * FPS + 1e-9)) + 1)
    c1 = int(round(upto_sec * 10))
    for i, s in enumerate(sessions):
        for c in range(sent["chunks"], c1):
            s.add_audio_chunk(wavs[i][c * CHUNK:(c + 1) * CHUNK], SR_IN)
        for f in range(sent["frames"], f1):
            s.add_frame(frames[i][f], timestamp=T0 + f / FPS)
    sent["frames"], sent["chunks"] = f1, c1
    return f1, c1


def clip_tick(now_sec, f1, c1):
    """The reference's tick on the existing path: per client, window from host buffers, host resample, batch 1."""
    rows = []
    lo = max(0, f1 - int(6.0 * FPS) - 1)
    for i in range(N):
        stamps = [f / FPS for f in range(lo, f1)]
        win = [lo + k for k, ts in enumerate(stamps) if ts >= now_sec - WINDOW] or list(range(lo, f1))
        idx = [win[k] for k in data.uniform_indices(len(win), T)]
        a1 = c1 * CHUNK
        wav16 = data.resample(wavs[i][max(0, a1 - int(SR_IN * WINDOW)):a1], SR_IN, 16000)
        clip = clips.video_clip_batch(clips._h2d(torch.from_numpy(frames[i][idx])[None], "cuda"))
        rows.append(runner.predict_probs(clip, torch.from_numpy(wav16)[None, None]))
    return torch.cat(rows)


feed(WINDOW)  # the buffers hold 3 s before the clock starts
times = {"pool": [], "clip_path": []}
worst = 0.0
base = dict(pool.stats)
for tick in range(M + 2):  # two warm-up ticks, not timed
    now_sec = WINDOW + (tick + 1) * STEP
    torch.cuda.synchronize()
    t = time.perf_counter()
    f1, c1 = feed(now_sec)
    res = pool.infer_ready(T0 + now_sec)
    torch.cuda.synchronize()
    t_pool = time.perf_counter() - t
    assert len(res) == N, (tick, len(res))
    t = time.perf_counter()
    want = clip_tick(now_sec, f1, c1)
    torch.cuda.synchronize()
    t_clip = time.perf_counter() - t
    got = torch.tensor([res[s.session_id]["probs"] for s in sessions])
    if args.grid == "window":  # the shared grid shows other frames: its rows are not the clip path's
        worst = max(worst, float((got - want).abs().max()))
    if tick == 1:
        base = dict(pool.stats)
    if tick >= 2:
        times["pool"].append(t_pool)
        times["clip_path"].append(t_clip)

d = {k: pool.stats[k] - base[k] for k in pool.stats}
out = {"sessions": N, "ticks": M, "grid": args.grid, "stride": args.stride if args.grid == "shared" else None}
for k, v in times.items():
    med = statistics.median(v)
    out[k] = {"tick_ms_median": round(med * 1e3, 3), "tick_ms_min": round(min(v) * 1e3, 3),
              "tick_ms_max": round(max(v) * 1e3, 3), "predictions_per_s": round(N / med, 1)}
out["pool"]["trunk_frames_per_prediction"] = round(d["frames_encoded"] / max(1, d["predictions"]), 3)
out["clip_path"]["trunk_frames_per_prediction"] = float(T)
out["max_abs_prob_diff_pool_vs_clip_path"] = worst if args.grid == "window" else None
print(json.dumps(out))
