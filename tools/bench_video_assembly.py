"""Time the video part of ``ClipLoader._assemble`` for one batch, per clip against batched: B = 32 clips of T = 8
cropped frames whose crop widths and heights are drawn between 200 and 500 pixels (a typical padded face box of a
1280 x 720 frame), the same decoded data in host memory for both.
  per clip: what ``device_video=False`` does -- per clip one pageable host-to-device copy and one resize launch, then
            the stack (eval) or the augmentation launch (train): 32 copies + 32 launches;
  batched:  ``device_video=True`` -- one copy of the batch's pinned buffer and one ``clips.crop_resize_frames``
            launch.  The gather of the crops into that pinned buffer (``ClipLoader._stage_video``) runs on the
            loader's producer thread, so it is not part of ``_assemble``; it is timed on its own (``stage_host_ms``,
            host clock) and once more inside the call (``batched_unstaged``).
All are timed with HIP events around the whole call (copies included: the stream waits for them) and with a host
clock around the call plus a device synchronise; 5 warm-up runs, then 30 alternating runs of each, medians.  The
outputs are compared bit for bit first.  Writes the JSON given by --out (default
profiles/clips/bench_video_assembly.json) and prints it.
    python tools/bench_video_assembly.py"""
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
from multimodalemotionrecognition_amd import clips  # noqa: E402
from multimodalemotionrecognition_amd import data as D  # noqa: E402

WARMUP, RUNS = 5, 30
B, T, SIZE = 32, 8, 112


def batch(seed=0):
    """``decoded`` as the loader's workers return it: (cropped frames [T, h, w, 3], ..., the video draws at [4])."""
    rng = np.random.default_rng(seed)
    decoded = []
    for _ in range(B):
        h, w = int(rng.integers(200, 501)), int(rng.integers(200, 501))
        decoded.append((rng.integers(0, 256, (T, h, w, 3), dtype=np.uint8), None, 0, {},
                        clips.draw_video_augment(rng)))
    return decoded


def once(loader, decoded, staged=None):
    """(device ms between two HIP events, wall ms including the synchronise, the video batch)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    video = loader._assemble_video(decoded, staged) if loader.device_video else per_clip(loader, decoded)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, video


def per_clip(self, decoded):
    """The video part of ``ClipLoader._assemble`` with ``device_video=False``, statement for statement."""
    if self.augment:
        u8 = torch.empty(len(decoded), self.T, self.size, self.size, 3, device=self.device, dtype=torch.uint8)
        for i, d in enumerate(decoded):
            clips.resize_frames_u8(torch.from_numpy(d[0]).to(self.device), self.size, out=u8[i])
        return clips.augment_clips(u8, [d[4] for d in decoded])
    vids = [clips.preprocess_frames(torch.from_numpy(d[0]).to(self.device), self.size) for d in decoded]
    return torch.stack(vids).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "clips" / "bench_video_assembly.json"))
    args = ap.parse_args()
    decoded = batch()
    nbytes = sum(d[0].nbytes for d in decoded)
    out = {"device": torch.cuda.get_device_name(0), "B": B, "T": T, "size": SIZE, "warmup": WARMUP, "runs": RUNS,
           "crop_side_range": [200, 500], "batch_mbytes": round(nbytes / 1e6, 2)}
    for split, augment in (("eval", False), ("train", True)):
        off = D.ClipLoader([], batch_size=B, num_frames=T, size=SIZE, augment=augment)
        on = D.ClipLoader([], batch_size=B, num_frames=T, size=SIZE, augment=augment, device_video=True)
        staged = on._stage_video(decoded)
        runs = {"per_clip": lambda: once(off, decoded), "batched": lambda: once(on, decoded, staged),
                "batched_unstaged": lambda: once(on, decoded)}
        ref = runs["per_clip"]()[2]
        for name in ("batched", "batched_unstaged"):
            assert torch.equal(runs[name]()[2], ref), "the two paths must give the same batch"
        for _ in range(WARMUP):
            for fn in runs.values():
                fn()
        ts = {name: ([], []) for name in runs}
        stage_ms = []
        for _ in range(RUNS):  # alternating: all see the same neighbours on the box
            for name, fn in runs.items():
                dev_ms, wall_ms, _ = fn()
                ts[name][0].append(dev_ms)
                ts[name][1].append(wall_ms)
            t0 = time.perf_counter()
            on._stage_video(decoded)
            stage_ms.append((time.perf_counter() - t0) * 1e3)
        res = {name: {"device_ms": round(statistics.median(d), 3), "wall_ms": round(statistics.median(w), 3),
                      "wall_ms_min_max": [round(min(w), 3), round(max(w), 3)]} for name, (d, w) in ts.items()}
        res["stage_host_ms"] = round(statistics.median(stage_ms), 3)
        res["per_clip_over_batched_wall"] = round(res["per_clip"]["wall_ms"] / res["batched"]["wall_ms"], 2)
        res["per_clip_over_batched_unstaged_wall"] = round(res["per_clip"]["wall_ms"] /
                                                           res["batched_unstaged"]["wall_ms"], 2)
        out[split] = res
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
