"""Emotion timeline over one recording (DESIGN.md "Timeline over a recording"): 30 s at 30 fps, 112 x 112 frames,
3 s windows every 1 s, 8 frames each -- xattn + WavLM + ResNet18, random-init weights, host inputs (the recording
crosses PCIe inside every timed call).  Three ways to the same 28 rows, interleaved round by round, median of the
rounds: ``predict_timeline`` on the shared grid, ``predict_timeline`` on the per-window grid, and the baseline a caller
had before: a loop of ``predict_probs`` over the windows cut out by hand (``video_clip_batch`` + waveform slice).
``batched`` is that loop's friendlier form, all windows stacked into one ``predict_probs`` call.
    python tools/bench_timeline.py [--seconds 30] [--fps 30] [--rounds 15]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from multimodalemotionrecognition_amd import clips  # noqa: E402
from multimodalemotionrecognition_amd.optimized_runtime import TorchModelRunner  # noqa: E402
from multimodalemotionrecognition_amd.timeline import plan_windows  # noqa: E402
from multimodalemotionrecognition_amd.train import build_model  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=int, default=30)
ap.add_argument("--fps", type=int, default=30)
ap.add_argument("--rounds", type=int, default=15)
args = ap.parse_args()

torch.manual_seed(0)
model = build_model(8, "xattn", pretrained_video=False, use_wavlm=True)
ck = {"model": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "val_f1": 0.0,
      "config": {"fusion": "xattn", "use_wavlm": True, "num_classes": 8}}
runner = TorchModelRunner(checkpoint=ck, device="cuda")
g = torch.Generator().manual_seed(20261020)
frames = torch.randint(0, 256, (args.seconds * args.fps, 112, 112, 3), generator=g, dtype=torch.uint8)
wav = (torch.rand(args.seconds * 16000, generator=g) - 0.5) * 0.5
plan = plan_windows(frames.shape[0], args.fps, wav.numel())
shared = plan_windows(frames.shape[0], args.fps, wav.numel(), frame_grid="shared")
wins = torch.stack([wav[s:s + plan.target] for s in plan.starts.tolist()])[:, None]


def loop():
    rows = []
    for w in range(plan.num_windows):
        clip = clips.video_clip_batch(clips._h2d(frames[plan.frame_idx[w].long()][None], "cuda"))
        rows.append(runner.predict_probs(clip, wins[w][None]))
    return torch.cat(rows)


def batched():
    clip = clips.video_clip_batch(clips._h2d(frames[plan.frame_idx.long()], "cuda"))
    return runner.predict_probs(clip, wins)


frames_d, wav_d, wins_d = frames.cuda(), wav.cuda(), wins.cuda()
idx_d = plan.frame_idx.long().cuda()


def batched_resident():
    return runner.predict_probs(clips.video_clip_batch(frames_d[idx_d]), wins_d)


ways = {"timeline_shared": lambda: runner.predict_timeline(frames, wav, args.fps, frame_grid="shared")["probs"],
        "timeline_window": lambda: runner.predict_timeline(frames, wav, args.fps)["probs"],
        "predict_probs_loop": loop, "predict_probs_batched": batched,
        # the same with the recording already on the device: no PCIe copy of the frames in the timed call
        "timeline_shared_resident":
            lambda: runner.predict_timeline(frames_d, wav_d, args.fps, frame_grid="shared")["probs"],
        "timeline_window_resident": lambda: runner.predict_timeline(frames_d, wav_d, args.fps)["probs"],
        "predict_probs_batched_resident": batched_resident}
last, times = {}, {k: [] for k in ways}
for rnd in range(3 + args.rounds):  # three warm-up rounds: first-call caches, then the graph captures
    for name, fn in ways.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last[name] = fn()  # ends in the probabilities' D2H copy
        torch.cuda.synchronize()
        if rnd >= 3:
            times[name].append((time.perf_counter() - t0) * 1e3)
out = {"config": f"{args.seconds} s at {args.fps} fps, 3 s windows every 1 s, 8 frames, xattn + WavLM + ResNet18",
       "windows": plan.num_windows, "frame_slots": int(plan.frame_idx.numel()),
       "trunk_frames": {"window": int(plan.unique_idx.numel()), "shared": int(shared.unique_idx.numel())},
       "rounds": args.rounds}
for name, ts in times.items():
    out[name] = {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}
out["max_abs_prob_diff_window_vs_loop"] = float((last["timeline_window"] - last["predict_probs_loop"]).abs().max())
out["max_abs_prob_diff_window_vs_batched"] = float((last["timeline_window"] - last["predict_probs_batched"]).abs().max())
out["max_abs_prob_diff_shared_vs_window"] = float((last["timeline_shared"] - last["timeline_window"]).abs().max())
out["rows_differ"] = bool(not torch.equal(last["timeline_window"][0], last["timeline_window"][1]))
print(json.dumps(out))
