#!/usr/bin/env python
"""Time the optimizer's per-step passes over FusedAdam's flat buffers (DESIGN.md "Optimizer: clipping, EMA, resume").

Default: build the benchmark's model (xattn fusion over ResNet18 + frozen WavLM, bench.py's C2 step) and its
optimizer, and time, with HIP events in ONE process, at that optimizer's flat-buffer sizes:

  adam       the existing mer_adam_step pass                      (28 B per parameter)   -- the yardstick
  norm       mer_grad_sqnorm + mer_clip_finalize                  ( 4 B per parameter)
  adam_ex    mer_adam_step_ex with the device coefficient + EMA   (36 B per parameter)

The three are run in turn, ``--rounds`` times, ``--iters`` back-to-back launches per timing window; the median over
rounds and the spread are printed, then the two ratios against ``adam``.  ``--numels a,b,...`` times given buffer
sizes instead of building the model.

``--train-step``: the same-box pair for the whole default xattn train step (bench.py's synthetic batch), clipping
off and on, alternating ``--rounds`` windows of ``--steps`` steps each; the spread over rounds stands beside it.
Prints one JSON line.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from multimodalemotionrecognition_amd import kernels as K  # noqa: E402

HP = (1e-3, 0.9, 0.999, 1e-8, 1e-4)


def c2_model():
    from multimodalemotionrecognition_amd.train import build_model

    torch.manual_seed(1234)
    return build_model(8, "xattn", pretrained_video=False, use_wavlm=True).cuda()


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3  # us per pass


def passes(numels, iters, rounds):
    g = torch.Generator(device="cuda").manual_seed(1)
    bufs = []
    for n in numels:
        p, grad = (torch.randn(n, device="cuda", generator=g) for _ in range(2))
        bufs.append(dict(p=p, g=grad * 1e-3, m=torch.zeros_like(p), v=torch.zeros_like(p), e=p.clone()))
    segs = K.NormSegments([b["g"] for b in bufs])
    rec = torch.zeros(K.CLIP_REC_FLOATS, device="cuda")
    coef = rec[K.CLIP_COEF:K.CLIP_COEF + 1]

    def adam():
        for b in bufs:
            K.adam_step(b["p"], b["g"], b["m"], b["v"], *HP, 10)

    def norm():
        K.grad_sqnorm(segs)
        K.clip_finalize(segs, 1.0, 1.0, rec)

    def adam_ex():
        for b in bufs:
            K.adam_step_ex(b["p"], b["g"], b["m"], b["v"], *HP, 10, coef=coef, ema=b["e"], ema_decay=0.999)

    fns = {"adam": adam, "norm": norm, "adam_ex": adam_ex}
    norm()  # the coefficient adam_ex reads
    for fn in fns.values():  # warm up: code objects loaded, buffers touched
        window(fn, 20)
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(window(fn, iters))
    out = {"numels": list(numels), "bytes_per_param": {"adam": 28, "norm": 4, "adam_ex": 36}, "iters": iters,
           "rounds": rounds}
    for k, v in times.items():
        out[k + "_us"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    base = out["adam_us"]["median"]
    out["norm_over_adam"] = round(out["norm_us"]["median"] / base, 3)
    out["adam_ex_over_adam"] = round(out["adam_ex_us"]["median"] / base, 3)
    total = sum(numels)
    for k, bpp in out["bytes_per_param"].items():
        out[k + "_TBps"] = round(total * bpp / (out[k + "_us"]["median"] * 1e-6) / 1e12, 3)
    return out


def train_step_pair(steps, rounds, warmup, max_norm):
    import bench
    from multimodalemotionrecognition_amd.train import TrainStep, build_optimizer, make_loss

    dev = torch.device("cuda", 0)
    runs = {}
    for name, mx in (("off", None), ("on", max_norm)):
        m = c2_model()
        opt = build_optimizer(m, lr=1e-3, weight_decay=1e-4, max_grad_norm=mx)
        step = TrainStep(m, opt, make_loss("xattn"), "xattn")
        video, audio, labels = bench.synthetic_batch(dev, 20261015)
        one = (lambda step=step, v=video, a=audio, y=labels: step(v, a, y, next_audio=a))
        for _ in range(warmup):
            one()
        torch.cuda.synchronize()
        runs[name] = one
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            times[k].append(window(fn, steps) / 1e3)  # ms per step
    out = {"steps_per_window": steps, "rounds": rounds, "max_grad_norm": max_norm}
    for k, v in times.items():
        out["clip_" + k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                                    "max": round(max(v), 4)}
    out["on_minus_off_ms"] = round(out["clip_on_ms"]["median"] - out["clip_off_ms"]["median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--numels", default=None, help="comma-separated flat-buffer sizes (default: the C2 optimizer's)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--train-step", action="store_true")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_passes.py measures on the GPU; none found")
    if args.train_step:
        print(json.dumps({"train_step": train_step_pair(args.steps, args.rounds, args.warmup, args.max_grad_norm)}))
        return
    if args.numels:
        numels = [int(x) for x in args.numels.split(",")]
    else:
        from multimodalemotionrecognition_amd.train import build_optimizer

        numels = [f.numel() for f in build_optimizer(c2_model()).flat_params()]
    print(json.dumps({"optim_passes": passes(numels, args.iters, args.rounds)}))


if __name__ == "__main__":
    main()
