"""North-star benchmark: 3 s-clip train steps/s (B=32 per GPU, xattn fusion) on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One step = the full reference train step (src/train.py:200-228) of FusionModel(mode='xattn') with
WavLM-base (frozen, forward) + ResNet18 trunk (train-mode BN, forward+backward) + xattn head
(forward+backward) + CrossEntropy + Adam, on one B=32 batch of synthetic 3 s clips
([32,8,3,112,112] frames, [32,1,48000] waveform) resident in HBM.  Weak scaling: each rank runs
B=32; `value` = steps completed by all ranks / wall time (max over ranks).

WavLM runs with the reference's train-mode semantics (the reference keeps the frozen WavLM in train mode
under no_grad, train.py:194): SpecAugment, dropout and LayerDrop -- so the algorithmic FLOPs of a step count
only the encoder layers actually executed; `wavlm_layers_per_step` reports them.

A plain run sets up, warms up, times the K steps, writes its outputs when ``--dump-outputs DIR`` is given
(`dump_outputs`: what the last timed step returned and left behind, as DIR/<name>.npy; the inputs and the initial
weights are seeded, so two builds run with the same arguments can be compared output for output) and prints the
result line.  Everything below takes runs of its own and is measured only with ``--full``.

Extra fields (``--full``): `roofline` for the dominant kernel (after the timed region: HIP events around `--probe-launches`
standalone launches of that kernel on its production shape, weights and stream, with nothing else in flight --
the figure a rocprofv3 kernel trace of the same command reports for it; the timed schedule is never altered),
`roofline_head` for the fused xattn head (HIP events around its graph replays in `--probe-steps` steps) and
`cpu_baseline` (the fp32 CPU oracle of the same step, rank 0, N=1: BASELINE.md section 3 -- warm-up steps,
then the median of timed steps, on the threads of this process's CPU share, CPU model recorded).

Multi-GPU: ``python bench.py --gpus N`` (N > 1) outside torchrun starts the N ranks itself -- one
``torch.distributed.run`` child job on 127.0.0.1, launched before this process imports torch or touches a GPU --
and exits with that job's status; rank 0 prints the one JSON line.  Under torchrun (WORLD_SIZE set) it runs as the
rank it was given and refuses to run when the group's size differs from ``--gpus``.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path


def _launch_ranks_if_needed(argv) -> None:
    """``--gpus N`` with N > 1 and no torchrun environment: run this script as an N-rank single-node job
    (python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1) and exit with its status.
    Called before torch is imported, so the parent never initialises a GPU (no exec: a child process)."""
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--gpus", type=int, default=1)
    known, _ = pre.parse_known_args(argv)
    if known.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    # --standalone: torchrun's own local rendezvous store binds a free port itself (no probe-then-close race for the
    # port); --local-addr 127.0.0.1: the ranks connect over loopback, whatever the container's hostname resolves to
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--nnodes=1",
           f"--nproc-per-node={known.gpus}", "--local-addr", "127.0.0.1", str(Path(__file__).resolve()), *argv]
    sys.exit(subprocess.run(cmd).returncode)


if __name__ == "__main__":
    _launch_ranks_if_needed(sys.argv[1:])

import torch  # noqa: E402
import torch.distributed as dist

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

from multimodalemotionrecognition_amd import fusion as F  # noqa: E402
from multimodalemotionrecognition_amd import kernels as K  # noqa: E402
from multimodalemotionrecognition_amd.dist import GradAllReduce, init_distributed, is_dist  # noqa: E402
from multimodalemotionrecognition_amd.train import (TrainStep, apply_two_stage_freeze_policy,  # noqa: E402
                                                    build_fusion_stage_optimizer, build_model, build_optimizer,
                                                    make_loss)

BATCH, FRAMES, SIZE, SAMPLES, CLASSES = 32, 8, 112, 48000, 8
PEAK_BF16_TFLOPS = 2500.0   # MI355X dense bf16 MFMA (MI355X_MICROARCH.md, spec)
PEAK_HBM_GBS = 8000.0       # HBM3E spec
# Dominant kernel (largest share of step time in profiles/): the WavLM feature-extractor conv1 as an
# implicit GEMM: M = B*4799 output frames, N = 512 channels, K = 3 taps * 512.
PROBE = ("gemm_bf16", (BATCH * 4799, 512, 1536))
# the kernel the train step's side-stream forward dispatches for that shape (gemm_bf16.hip, CU-time rule -2: the
# split ring, 1,200 tiles of 256x256, 16 waves each; PipeCfg's last two flags: operand-swapped with bf16 epilogue
# staging, LDS-DMA issued between MFMA rows -- v23)
PROBE_KERNEL = "gemm_pipe_kernel<PipeCfg<256,256,4,4,2,64,3,1,1>, bf16>"
PMC_FILE = ROOT / "profiles" / "pmc_traffic.json"
PMC_HEAD_FILE = ROOT / "profiles" / "pmc_traffic_head.json"  # tools/pmc_head.py summarize (fused head fwd + bwd)
# Algorithmic work per clip: ResNet18 fwd+bwd over 8 frames 22.8 GFLOP, head fwd+bwd 0.141, WavLM
# feature extractor 14.72 + pos-conv 1.42 + projection 0.12, and 2.177 GFLOP per EXECUTED encoder layer
# (projections 0.703 + FFN 1.406 + attention 0.068; LayerDrop skips ~1.1 of 12 in train mode).
STEP_GFLOP_PER_CLIP_FIXED = 22.8 + 0.141 + 14.72 + 1.42 + 0.12
WAVLM_LAYER_GFLOP_PER_CLIP = 0.703 + 1.406 + 0.068
# the fused xattn head's arithmetic (csrc/xattn_fused*.hip): fp32-class products as three bf16 MFMA passes, so its
# MFMA peak is the box's dense bf16 peak / 3 (box_peaks)


def head_flop(B=BATCH, T=FRAMES, Ta=149, sd=768, vd=512, d=128, h1=256, c=CLASSES):
    """Algorithmic FLOPs of the xattn head forward + backward (fusion.py:366-411): every Linear 2MNK forward,
    dX + dW backward (no dX for audio_seq_proj: the frozen WavLM needs none), the two attentions' QK^T and PV."""
    lin = [(B * Ta, d, sd), (B * Ta, d, d), (B * T, d, vd), (B * T, d, d), (B * Ta, 2 * d, d), (B * T, d, d),
           (B * Ta, d, d), (B * T, 2 * d, d), (B * Ta, d, d), (B, h1, 2 * d), (B, c, h1)]
    fwd = sum(2.0 * m * n * k for m, n, k in lin) + 2 * 2 * (2.0 * B * T * Ta * d)
    return fwd + 2 * fwd - 2.0 * B * Ta * d * sd


def pmc_traffic():
    """HBM bytes per launch of the probe kernel from the committed PMC passes (tools/pmc_traffic.py:
    FETCH_SIZE x2 (gfx950 correction) + WRITE_SIZE, rocprofv3 --pmc in separate passes), or None when
    no measurement of the current probe kernel is on file."""
    try:
        d = json.loads(PMC_FILE.read_text())
    except (OSError, ValueError):
        return None
    if d.get("kernel_match") not in PROBE_KERNEL.replace(" ", "") or tuple(d.get("shape", ())) != PROBE[1]:
        return None
    return d.get("traffic_bytes_per_launch")


def pmc_traffic_head():
    """HBM bytes of one fused-head forward + backward from the committed PMC passes (tools/pmc_head.py), or None."""
    try:
        return json.loads(PMC_HEAD_FILE.read_text()).get("traffic_bytes_per_step")
    except (OSError, ValueError):
        return None


def synthetic_batch(device, seed):
    """ravdess.py:386-389,505-513 layouts: ImageNet-normalised frames, waveform in [-1,1], labels."""
    g = torch.Generator(device=device).manual_seed(seed)
    mean = torch.tensor([0.485, 0.456, 0.406], device=device).view(1, 1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device=device).view(1, 1, 3, 1, 1)
    video = (torch.rand(BATCH, FRAMES, 3, SIZE, SIZE, device=device, generator=g) - mean) / std
    audio = (0.1 * torch.randn(BATCH, 1, SAMPLES, device=device, generator=g)).clamp_(-1, 1)
    labels = torch.randint(0, CLASSES, (BATCH,), device=device, generator=g)
    return video.contiguous(), audio.contiguous(), labels


DUMP_SAMPLE = 1 << 18  # elements kept of a larger array (a fixed, seeded sample): the whole dump stays well below 64 MB


def dump_outputs(out_dir, arrays):
    """``--dump-outputs DIR``: write ``arrays`` ({name: tensor}) as DIR/<name>.npy, float32 (float64 for float64 and
    integer tensors).  An array of more than DUMP_SAMPLE elements is written as the sample at seeded, sorted flat
    indices that depend on its name's position and its size alone, so two builds write the same elements."""
    import numpy as np

    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    total = 0
    for i, (name, t) in enumerate(arrays.items()):
        t = t.detach()
        t = t.to(torch.float32 if t.is_floating_point() and t.dtype != torch.float64 else torch.float64)
        a = t.cpu().numpy()
        if a.size > DUMP_SAMPLE:
            idx = np.sort(np.random.default_rng(1000 + i).choice(a.size, DUMP_SAMPLE, replace=False))
            a = a.reshape(-1)[idx]
        total += a.nbytes
        assert total <= 64 << 20, "dump_outputs: more than 64 MB"
        np.save(out_dir / f"{name}.npy", np.ascontiguousarray(a))


def step_outputs(model, loss, preds):
    """What a caller of one ``TrainStep`` receives: the returned loss and top-1 predictions, and the state the step
    left in the model -- every trainable parameter after Adam and the floating-point buffers (BatchNorm running
    statistics).  Frozen parameters are unchanged by the step and are left out."""
    arrays = {"loss": loss.reshape(1), "preds": preds}
    for n, p in model.named_parameters():
        if p.requires_grad:
            arrays["param." + n] = p
    for n, b in model.named_buffers():
        if b.is_floating_point():
            arrays["buffer." + n] = b
    return arrays


def box_peaks():
    """The MI355X's dense MFMA and HBM peaks, from the box itself: compute units and the
    peak engine clock from rocminfo / the device properties; dense bf16 = CUs x 4 SIMDs x 1,024 FLOP/clk (the
    v_mfma_f32_32x32x16_bf16 rate, MI355X_MICROARCH.md) x clock.  HBM bandwidth is not reported by the runtime:
    the 8 TB/s HBM3E spec is used and labelled as such."""
    import subprocess

    cus, mhz, src = 0, 0.0, []
    try:
        prop = torch.cuda.get_device_properties(0)
        cus = int(prop.multi_processor_count)
        src.append("torch device properties (CUs)")
    except Exception:  # noqa: BLE001
        pass
    try:
        txt = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=30).stdout
        agent = None
        for line in txt.splitlines():
            t = line.strip()
            if t.startswith("Name:") and "gfx" in t:
                agent = t.split(":", 1)[1].strip()
            if agent and t.startswith("Max Clock Freq. (MHz):"):
                mhz = float(t.split(":", 1)[1].split()[0])
            if agent and t.startswith("Compute Unit:") and not cus:
                cus = int(t.split(":", 1)[1].split()[0])
            if agent and mhz:
                break
        if mhz:
            src.append(f"rocminfo ({agent}: max clock)")
    except Exception:  # noqa: BLE001
        pass
    out = {"cus": cus or None, "max_sclk_mhz": mhz or None, "source": ", ".join(src) or "spec",
           "bf16_dense_tflops": PEAK_BF16_TFLOPS, "hbm_gbs": PEAK_HBM_GBS, "hbm_source": "HBM3E spec (8 TB/s)"}
    if cus and mhz:
        out["bf16_dense_tflops"] = round(cus * 4 * 1024 * mhz * 1e6 / 1e12, 1)
    return out


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_share_threads() -> int:
    """Threads of this process's CPU share: OMP_NUM_THREADS when the launcher set it (the GPU box sets it to its
    16-CPU share; os.cpu_count() there reports the whole machine), else the affinity set."""
    env = os.environ.get("OMP_NUM_THREADS")
    if env and env.isdigit() and int(env) > 0:
        return int(env)
    return len(os.sched_getaffinity(0))


def cpu_baseline(threads: int, steps: int = 10, warmup: int = 10):
    """The fp32 CPU oracle of the same train step at B=32 (test infrastructure, timed as the baseline):
    ``warmup`` untimed steps, then the median of ``steps`` timed ones."""
    import statistics

    from oracle import params as OP
    from oracle import fusion_ref, resnet18_ref, train_ref, wavlm_ref

    torch.set_num_threads(threads)
    shapes = [("video_model." + n, s) for n, s in resnet18_ref.param_shapes()]
    shapes += [("audio_model.wavlm." + n, s) for n, s in wavlm_ref.wavlm_param_shapes()]
    shapes += fusion_ref.xattn_head_param_shapes()
    p = {k: torch.from_numpy(v) for k, v in OP.init_state(shapes).items()}
    trainable = [k for k in p if (k.startswith("video_model.") and not k.endswith(
        ("running_mean", "running_var", "num_batches_tracked"))) or
        (not k.startswith(("video_model.", "audio_model.")) and not k.startswith("audio_time_conv"))]
    for k in trainable:
        p[k].requires_grad_(True)
    opt = train_ref.AdamRef([p[k] for k in trainable], lr=1e-3, weight_decay=1e-4)
    video, audio, labels = OP.clip_inputs(BATCH)
    video, audio, labels = torch.from_numpy(video), torch.from_numpy(audio), torch.from_numpy(labels)
    for _ in range(warmup):
        train_ref.train_step(p, trainable, opt, video, audio, labels)
    times = []
    for _ in range(steps):
        t = time.perf_counter()
        train_ref.train_step(p, trainable, opt, video, audio, labels)
        times.append(time.perf_counter() - t)
    dt = statistics.median(times)
    return {"value": round(1.0 / dt, 4), "unit": "steps/s", "cores": threads, "kind": "port",
            "cpu_model": cpu_model(), "os_cpu_count": os.cpu_count(),
            "sample": f"median of {steps} timed steps after {warmup} warm-up steps of the fp32 oracle train step at "
                      f"B=32 ({dt:.2f} s/step, {BATCH / dt:.2f} clips/s), torch CPU eager, {threads} threads"}


def time_dominant(model, dev, probe, launches: int):
    """HIP events around standalone launches of the WavLM conv1 implicit GEMM (wavlm_audio._conv_layer, i = 1) on
    its production shape, bf16 weight pack and stream, operands resident in HBM, nothing else in flight."""
    wav = model.audio_model.wavlm
    L0 = (SAMPLES - 10) // 5 + 1          # conv0 output frames (kernel 10, stride 5)
    L1 = (L0 - 3) // 2 + 1                # conv1 output frames (kernel 3, stride 2)
    M, N, Kd = PROBE[1]
    assert M == BATCH * L1 and N == 512 and Kd == 3 * 512
    x = (torch.rand(BATCH, L0, 512, device=dev) * 2 - 1).bfloat16()
    y = torch.empty(BATCH, L1, 512, device=dev, dtype=torch.bfloat16)
    w = wav.packed_weights()["conv"][0]

    def launch():
        # the train step's tile rule (wavlm_audio._gemm_pick: -2 in the train-mode forward)
        K.gemm_bf16(x, w, y, M=M, K=Kd, rows=(L1, 2 * 512, L0 * 512), act="gelu", variant=-2)

    with torch.cuda.stream(F._side_stream(dev)):  # the stream the production WavLM forward runs on
        for _ in range(3):
            launch()
        probe.active = True
        K.PROBE = probe
        for _ in range(launches):
            launch()
        K.PROBE = None
        probe.active = False
    torch.cuda.synchronize()


CORE_KERNELS = ("xh_v2a_fwd", "xh_a2v_fwd", "xh_v2a_bwd", "xh_a2v_bwd")


def core_attention(B=BATCH, T=FRAMES, Ta=149, d=128, H=4):
    """(FLOP, bytes) of the xattn attention cores (fusion.py:394,398: v2a and a2v nn.MultiheadAttention) per train
    step: forward QK^T + PV per direction, backward dP, dV, dQ, dK (2x); bytes = Q, K, V read and P, O written in
    the forward, Q, K, V, P, dO read and dQ, dK, dV written in the backward, fp32."""
    flop = 3 * 2 * (2 * 2.0 * B * T * Ta * d)  # two directions x (fwd 2 products + bwd 4)
    byt = 0
    for lq, lk in ((T, Ta), (Ta, T)):
        q, kv, p, o = B * lq * d * 4, B * lk * 2 * d * 4, B * H * lq * lk * 4, B * lq * d * 4
        byt += (q + kv + p + o) + (q + kv + p + o) + (q + kv)
    return flop, byt


def roof_core(core_ms, peak_split):
    """The ``roofline_head.core`` entry: the attention cores' FLOPs over the summed standalone durations of the
    four kernels that run them, against min(split-bf16 peak, intensity x HBM bandwidth)."""
    if not core_ms or any(v is None for v in core_ms.values()):
        return None
    flop, byt = core_attention()
    ms = sum(core_ms.values())
    ai = flop / byt
    attain = min(peak_split, ai * PEAK_HBM_GBS / 1e3)
    ach = flop / (ms * 1e-3) / 1e12
    return {"bound": "mfma" if peak_split < ai * PEAK_HBM_GBS / 1e3 else "hbm", "achieved": round(ach, 3),
            "peak": round(attain, 2), "unit": "TFLOP/s", "frac": round(ach / attain, 4), "algorithmic_flop": flop,
            "algorithmic_bytes": byt, "intensity_flop_per_byte": round(ai, 2), "kernel_ms": {
                k: round(v, 4) for k, v in core_ms.items()}, "ms": round(ms, 4),
            "measured": "HIP events around 20 eager train-mode head fwd+bwd passes per kernel (each kernel also "
                        "runs its out-projection, residual + LayerNorm; the whole duration is charged to the core)"}


CORE_ATTN_FILE = Path(__file__).resolve().parent / "profiles" / "r06" / "core_attn.json"


def roof_core_attn(peak_split):
    """The ``roofline_head.core_attn`` entry: the attention cores' FLOPs over the QK^T / softmax / PV phases alone
    (their backward too) -- phase stamps of the timing build (tools/xt_phases.py ... core), committed as
    profiles/r06/core_attn.json; the four kernels' out-projection / residual / LayerNorm phases are excluded."""
    if not CORE_ATTN_FILE.exists():
        return None
    rec = json.loads(CORE_ATTN_FILE.read_text())
    flop, byt = core_attention()
    ms = rec["core_attn_us"] / 1e3
    ai = flop / byt
    attain = min(peak_split, ai * PEAK_HBM_GBS / 1e3)
    ach = flop / (ms * 1e-3) / 1e12
    return {"bound": "mfma" if peak_split < ai * PEAK_HBM_GBS / 1e3 else "hbm", "achieved": round(ach, 3),
            "peak": round(attain, 2), "unit": "TFLOP/s", "frac": round(ach / attain, 4), "ms": round(ms, 4),
            "kernel_us": {k: v["core_us"] for k, v in rec["kernels"].items()},
            "source": "profiles/r06/core_attn.json (" + rec["method"] + ")"}


def time_head_core(model, dev, reps: int):
    """HIP events around every launch of the fused head's four attention kernels (F2 / F3 forward, G2 / G3 backward:
    each fuses its attention with the out-projection, drop-path + residual + LayerNorm and, F2 / G2, the next
    projection) in eager train-mode head forward + backward passes on the production shapes, nothing else in
    flight.  Returns {kernel: avg ms}."""
    from multimodalemotionrecognition_amd import xattn_head as XH

    names, params = model.head_params()
    p = dict(zip(names, params))
    cfg = model.head_config()
    g = torch.Generator(device=dev).manual_seed(7)
    v = torch.randn(BATCH, FRAMES, 512, device=dev, generator=g)
    a = torch.randn(BATCH, 149, 768, device=dev, generator=g).to(torch.bfloat16)
    rng = torch.full((1,), 4242, dtype=torch.int64, device=dev)
    used = set(XH.used_param_names(cfg))
    grads = {n: torch.zeros_like(t) for n, t in p.items() if n in used}
    dl = torch.randn(BATCH, CLASSES, device=dev, generator=g)
    probe = K.MultiProbe(CORE_KERNELS)

    def one():
        _, ctx = XH.head_forward(p, cfg, v, a, True, rng)
        XH.head_backward(p, ctx, dl, grads, need_dv_feat=True)

    with torch.no_grad():
        for _ in range(3):
            one()
        torch.cuda.synchronize()
        probe.active = True
        K.PROBE = probe
        for _ in range(reps):
            one()
        K.PROBE = None
        probe.active = False
    torch.cuda.synchronize()
    return {n: probe.avg_ms(n) for n in CORE_KERNELS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure the rooflines (probe steps and launches, box peaks) and "
                         "the CPU baseline; a plain run times its steps and prints the result line only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last timed step computed as DIR/<name>.npy")
    ap.add_argument("--probe-steps", type=int, default=10,
                    help="(--full) instrumented steps after the timed region in which the fused head's graphs are timed")
    ap.add_argument("--probe-launches", type=int, default=20,
                    help="(--full) standalone launches of the dominant kernel timed after the timed region")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline")
    ap.add_argument("--cpu-threads", type=int, default=0, help="0: this process's CPU share (cpu_share_threads)")
    ap.add_argument("--cpu-steps", type=int, default=10)
    ap.add_argument("--cpu-warmup", type=int, default=10)
    ap.add_argument("--stream-priority", choices=("normal", "high"), default="normal",
                    help="run the training loop on a stream of this priority (the prefetched WavLM forward stays on its "
                         "normal-priority side stream)")
    ap.add_argument("--no-prefetch", action="store_true",
                    help="run the frozen WavLM inline in every step instead of overlapping the next batch's "
                         "WavLM forward with this step's backward")
    ap.add_argument("--emotion-prior", action="store_true",
                    help="xattn with the emotion-prior attention bias (C4 variant, not the headline config)")
    ap.add_argument("--c5", action="store_true",
                    help="BASELINE.json configs[4] instead: the inference_worker batch path (TorchModelRunner."
                         "predict_probs, B=64 3 s clips) bf16 vs INT8, clips/s, top-1 agreement, B=64 CPU baseline")
    ap.add_argument("--wavlm-unfreeze", type=int, default=0,
                    help="stage-2 fine-tuning step instead (train.py:798-872 two-stage policy): unfreeze the last N "
                         "WavLM layers and the last video block, stage optimizer groups (not the headline config)")
    ap.add_argument("--stub-step", action="store_true",
                    help="test hook for the rank launcher: a CPU matmul + gloo all-reduce in place of the train step")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:  # the plain run: nothing but the timed steps
        args.probe_steps = args.probe_launches = 0
        args.no_cpu_baseline = True

    world, rank, local = init_distributed("gloo" if args.stub_step else None)
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but the process group has {world} rank(s)", file=sys.stderr, flush=True)
        sys.exit(2)
    if args.stub_step:
        return _bench_stub(args, world, rank)
    if args.c5:
        return _bench_c5(args, world, rank, local)
    if args.stream_priority == "high":
        hi = torch.cuda.Stream(device=local, priority=torch.cuda.Stream.priority_range()[1])
        with torch.cuda.stream(hi):
            return _bench(args, world, rank, local)
    return _bench(args, world, rank, local)


def dp_fields(local_step_ms, sync, dev):
    """The DP diagnostics of the bench line: per rank its own step time and the ``CommTimes``
    summary of its ``GradAllReduce`` (exposed all-reduce ms per step, how early the head + layer4 bucket went out
    before the backward's end), all-gathered to every rank; rank 0 reports them with the max and min over ranks, so
    a shortfall of the 1 -> 8 curve can be traced to communication or to a slow rank from the run's own line."""
    s = sync.times.summary() if sync is not None and sync.times is not None else {}
    nan = float("nan")
    vec = torch.tensor([local_step_ms, s.get("allreduce_exposed_ms") or nan, s.get("early_bucket_lead_ms") or nan,
                        float(s.get("early_bucket_steps", 0)), float(s.get("steps", 0))], device=dev,
                       dtype=torch.float64)
    world = dist.get_world_size() if is_dist() else 1
    rows = [torch.zeros_like(vec) for _ in range(world)]
    if is_dist():
        dist.all_gather(rows, vec)
    else:
        rows = [vec]
    keys = ("step_ms", "allreduce_exposed_ms", "early_bucket_lead_ms", "early_bucket_steps", "timed_steps")
    per = []
    for r, row in enumerate(rows):
        d = {"rank": r}
        for k, v in zip(keys, row.tolist()):
            d[k] = None if v != v else (int(v) if k.endswith("steps") else round(v, 4))
        per.append(d)
    agg = {}
    for k in keys[:3]:
        vals = [d[k] for d in per if d[k] is not None]
        agg[k] = {"max": max(vals), "min": min(vals)} if vals else None
    return {"per_rank": per, "over_ranks": agg,
            "bytes_allreduced_per_step": sum(f.numel() * f.element_size() for f in sync.opt.flat_grads())
            if sync is not None else None,
            "measured": "HIP events on the compute stream (host clock under gloo/CPU): early-bucket hook, backward "
                        "end, and around the waits on the launched all-reduces; means over the timed steps"}


def _bench_stub(args, world, rank):
    """The launcher's test hook (tests/test_bench_launch_cpu.py): the same warm-up / barrier / timed region /
    max-over-ranks structure as ``_bench`` around a CPU matmul and the real ``GradAllReduce`` (gloo, FusedAdam's
    flat buffers of a small model, the early-bucket hook fired mid-step), one JSON line from rank 0 that says how
    many ranks took part, with the same ``dp`` diagnostics as the train-step line."""
    from multimodalemotionrecognition_amd.optim import FusedAdam

    x = torch.full((64, 64), 1.0 / 64)
    m = torch.nn.Sequential(torch.nn.Linear(64, 64), torch.nn.Linear(64, 8))
    opt = FusedAdam(list(m.parameters()))
    sync = GradAllReduce(opt, model=m, early_params=list(m[1].parameters()), mask_sync=False, timing=True) \
        if is_dist() else None
    (flat,) = opt.flat_grads()

    def one():
        nonlocal x
        x = x @ x
        flat.fill_(1.0)
        if sync is not None:
            sync.grads_ready()  # the early bucket, then the rest of the "backward"
            x = x @ x
            sync()

    for _ in range(args.warmup):
        one()
    if sync is not None:
        sync.times.reset()
    if is_dist():
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one()
    local_ms = (time.perf_counter() - t0) / max(1, args.steps) * 1e3
    if is_dist():
        dist.barrier()
    el = torch.tensor([time.perf_counter() - t0])
    ranks = torch.ones(1)
    if is_dist():
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
        dist.all_reduce(ranks)
    dp = dp_fields(local_ms, sync, torch.device("cpu"))
    if rank == 0:
        print(json.dumps({"metric": "stub", "value": round(world * args.steps / float(el), 3), "unit": "steps/s",
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ranks_reporting": int(ranks), "pid": os.getpid(), "dp": dp}), flush=True)
    if is_dist():
        dist.barrier()
        dist.destroy_process_group()


def cpu_baseline_c5(threads: int, batch: int = 64, steps: int = 2, warmup: int = 1):
    """The fp32 CPU oracle of the C5 batch (encoders in eval mode + xattn head + softmax) at B=64."""
    import statistics

    from oracle import params as OP
    from oracle import fusion_ref, resnet18_ref, train_ref, wavlm_ref

    torch.set_num_threads(threads)
    shapes = [("video_model." + n, s) for n, s in resnet18_ref.param_shapes()]
    shapes += [("audio_model.wavlm." + n, s) for n, s in wavlm_ref.wavlm_param_shapes()]
    shapes += fusion_ref.xattn_head_param_shapes()
    p = {k: torch.from_numpy(v) for k, v in OP.init_state(shapes).items()}
    video, audio, _ = OP.clip_inputs(batch)
    video, audio = torch.from_numpy(video), torch.from_numpy(audio)

    def run():
        with torch.no_grad():
            return torch.softmax(train_ref.model_forward(p, video, audio, bn_training=False), dim=1)

    for _ in range(warmup):
        run()
    times = []
    for _ in range(steps):
        t = time.perf_counter()
        run()
        times.append(time.perf_counter() - t)
    dt = statistics.median(times)
    return {"value": round(batch / dt, 3), "unit": "clips/s", "cores": threads, "kind": "port",
            "cpu_model": cpu_model(), "os_cpu_count": os.cpu_count(),
            "sample": f"median of {steps} B={batch} fp32 oracle forwards (eval) after {warmup} warm-up "
                      f"({dt:.2f} s/batch), torch CPU eager, {threads} threads"}


def _bench_c5(args, world, rank, local):
    """BASELINE.json configs[4]: inference_worker.py:131-147 -> TorchModelRunner.predict_probs
    (optimized_runtime.py:95-108) on B=64 synthetic 3 s clips resident on the GPU; bf16 encoders with the fp32 head
    vs the INT8 dynamic-quantised Linears; the probabilities' D2H copy (the reference's .cpu()) is inside the
    timed region.  Replicas only (no collective on the inference path): value = clips of all ranks / max time."""
    from multimodalemotionrecognition_amd.optimized_runtime import TorchModelRunner

    dev = torch.device("cuda", local)
    B = 64
    torch.manual_seed(0)
    model = build_model(CLASSES, "xattn", pretrained_video=False, use_wavlm=True)
    ck = {"model": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "val_f1": 0.0,
          "config": {"fusion": "xattn", "use_wavlm": True, "num_classes": CLASSES}}
    del model
    g = torch.Generator(device=dev).manual_seed(20261015 + rank)
    mean = torch.tensor([0.485, 0.456, 0.406], device=dev).view(1, 1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device=dev).view(1, 1, 3, 1, 1)
    video = ((torch.rand(B, FRAMES, 3, SIZE, SIZE, device=dev, generator=g) - mean) / std).contiguous()
    audio = (0.1 * torch.randn(B, 1, SAMPLES, device=dev, generator=g)).clamp_(-1, 1).contiguous()
    res, probs = {}, {}
    for name, q in (("bf16", False), ("int8", True)):
        runner = TorchModelRunner(checkpoint=ck, device=str(dev), enable_dynamic_quant=q)
        for _ in range(args.warmup):
            runner.predict_probs(video, audio)
        torch.cuda.synchronize()
        if is_dist():
            dist.barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            pr = runner.predict_probs(video, audio)
        torch.cuda.synchronize()
        el = torch.tensor([time.perf_counter() - t0], device=dev)
        if is_dist():
            dist.all_reduce(el, op=dist.ReduceOp.MAX)
        el = float(el)
        probs[name] = pr
        res[name] = {"clips_per_s": round(world * B * args.steps / el, 1), "ms_per_batch": round(el / args.steps * 1e3, 3)}
        del runner
    agree = float((probs["int8"].argmax(1) == probs["bf16"].argmax(1)).float().mean())
    out = {
        "metric": "inference_worker batch clips/s (B=64, xattn, bf16 and INT8 Linears)",
        "value": res["bf16"]["clips_per_s"], "unit": "clips/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": res["bf16"]["ms_per_batch"], "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
        "data": "synthetic (seeded B=64 3 s clips resident in HBM; random-init weights)",
        "config": {"workload": "TorchModelRunner.predict_probs, ResNet18 + WavLM-base + xattn head (eval)",
                   "per_gpu_batch": B, "parallelism": f"replicas{world}"},
        "bf16": res["bf16"], "int8": res["int8"], "top1_agreement_int8_vs_bf16": agree,
        "max_abs_prob_diff_int8_vs_bf16": round(float((probs["int8"] - probs["bf16"]).abs().max()), 6),
        "peaks": box_peaks() if args.full else None, "cpu_baseline": None,
    }
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"probs_" + k: v for k, v in probs.items()})
    if world == 1 and not args.no_cpu_baseline:
        threads = args.cpu_threads if args.cpu_threads > 0 else cpu_share_threads()
        out["cpu_baseline"] = cpu_baseline_c5(threads)
    print(json.dumps(out), flush=True)
    if is_dist():
        dist.barrier()
        dist.destroy_process_group()


def _bench(args, world, rank, local):
    dev = torch.device("cuda", local)
    torch.manual_seed(1234)  # identical init on every rank
    prior = dict(xattn_use_emotion_prior=True, forward_emotion_prior_flags=True) if args.emotion_prior else {}
    model = build_model(CLASSES, "xattn", pretrained_video=False, use_wavlm=True, **prior).to(dev)
    if args.wavlm_unfreeze > 0:
        apply_two_stage_freeze_policy(model, stage=2, unfreeze_wavlm_layers=args.wavlm_unfreeze)
        opt = build_fusion_stage_optimizer(model, stage=2, lr=1e-3, weight_decay=1e-4)
    else:
        opt = build_optimizer(model, lr=1e-3, weight_decay=1e-4)
    sync = GradAllReduce(opt, model=model, timing=True) if is_dist() else None
    step = TrainStep(model, opt, make_loss("xattn"), "xattn", sync)
    video, audio, labels = synthetic_batch(dev, 20261015 + rank)

    # The synthetic stream repeats one resident batch, so the next step's waveform is `audio` itself:
    # each step still runs exactly one WavLM forward (the next batch's, overlapping its own backward).
    nxt = None if args.no_prefetch else audio
    for _ in range(args.warmup):
        step(video, audio, labels, next_audio=nxt)
    torch.cuda.synchronize()

    wav = model.audio_model.wavlm
    lay0, fwd0 = wav.executed_layers, wav.train_forwards
    if sync is not None:
        sync.times.reset()  # the DP diagnostics cover the timed steps only
    if is_dist():
        dist.barrier()
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    loss = last = None
    for i in range(args.steps):
        last = step(video, audio, labels, next_audio=nxt)
        marks[i + 1].record()
    loss = last[0]
    torch.cuda.synchronize()
    local_ms = (time.perf_counter() - t0) / args.steps * 1e3  # this rank alone, before the closing barrier
    if is_dist():
        dist.barrier()
    elapsed = time.perf_counter() - t0
    step_ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
    median_ms = step_ms[len(step_ms) // 2] if len(step_ms) % 2 else 0.5 * (step_ms[len(step_ms) // 2 - 1] +
                                                                           step_ms[len(step_ms) // 2])
    layers = (wav.executed_layers - lay0) / max(1, wav.train_forwards - fwd0)
    dp = dp_fields(local_ms, sync, dev) if is_dist() else None
    if args.dump_outputs and rank == 0:  # before any probe step runs the optimizer again
        dump_outputs(args.dump_outputs, step_outputs(model, *last))

    # probe steps (after the timed region): the fused head's forward / backward graph replays bracketed by HIP
    # events on their stream
    hprobe = F.HeadProbe()
    if args.probe_steps > 0:
        F.HEAD_PROBE = hprobe
        for _ in range(args.probe_steps):
            step(video, audio, labels, next_audio=nxt)
        torch.cuda.synchronize()
        F.HEAD_PROBE = None
    # the dominant kernel: standalone launches on the production conv1 shape / weight pack / WavLM stream
    probe = K.KernelProbe(PROBE[0], PROBE[1], units=2.0 * PROBE[1][0] * PROBE[1][1] * PROBE[1][2])
    if args.probe_launches > 0:
        time_dominant(model, dev, probe, args.probe_launches)
    kms = probe.avg_ms()
    peaks = box_peaks() if args.full else None  # (asks rocminfo: a child process)
    peak_bf16 = peaks["bf16_dense_tflops"] if peaks else PEAK_BF16_TFLOPS
    peak_split = peak_bf16 / 3
    roof = None
    if kms:
        achieved = probe.units / (kms * 1e-3) / 1e12
        roof = {"bound": "mfma", "achieved": round(achieved, 1), "peak": peak_bf16, "unit": "TFLOP/s",
                "frac": round(achieved / peak_bf16, 4), "traffic": pmc_traffic(),
                "kernel": f"{PROBE_KERNEL} (WavLM conv1 implicit GEMM {PROBE[1][0]}x{PROBE[1][1]}x{PROBE[1][2]})",
                "avg_ms": round(kms, 4), "launches": len(probe.pairs),
                "measured": f"HIP events around {len(probe.pairs)} standalone launches after the timed region "
                            "(production shape, weight pack and stream)"}
    core_ms = time_head_core(model, dev, 20) if (args.probe_launches > 0 and args.wavlm_unfreeze == 0
                                                 and not args.emotion_prior) else None
    roof_head = None
    hms = hprobe.avg_ms()
    if hms and args.wavlm_unfreeze == 0 and not args.emotion_prior:
        # the fused head's forward + backward graph replays in production (with the next batch's WavLM running
        # beside them on the prefetch stream); bytes = the saved activations (inputs included) written once and
        # read once + the used head parameters read twice and their gradients written once + dv_feat
        fwd_ms, bwd_ms = hms
        head_ms = fwd_ms + bwd_ms
        hparams = sum(t.numel() for n, t in zip(*model.head_params()) if t.requires_grad)
        hbytes = 2 * hprobe.saved_bytes + 3 * 4 * hparams + 4 * BATCH * FRAMES * 512
        hflop = head_flop()
        ai = hflop / hbytes
        attain = min(peak_split, ai * PEAK_HBM_GBS / 1e3)
        ach = hflop / (head_ms * 1e-3) / 1e12
        roof_head = {"bound": "mfma" if peak_split < ai * PEAK_HBM_GBS / 1e3 else "hbm",
                     "achieved": round(ach, 2), "peak": round(attain, 1), "unit": "TFLOP/s",
                     "frac": round(ach / attain, 4), "traffic": pmc_traffic_head(),
                     "kernel": "fused xattn head fwd+bwd (csrc/xattn_fused.hip F1-F4, xattn_fused_bwd.hip G1-G4 + W)",
                     "algorithmic_flop": hflop, "algorithmic_bytes": hbytes, "intensity_flop_per_byte": round(ai, 2),
                     "fwd_ms": round(fwd_ms, 4), "bwd_ms": round(bwd_ms, 4), "ms_per_step": round(head_ms, 4),
                     "hbm_gbs_achieved": round(hbytes / (head_ms * 1e-3) / 1e9, 1),
                     "peak_basis": "min(split-bf16 fp32-class MFMA peak = 2.5 PF / 3, intensity x 8 TB/s)",
                     "core": roof_core(core_ms, peak_split),
                     "core_attn": roof_core_attn(peak_split),
                     "measured": f"HIP events around the head's forward / backward graph replays in "
                                 f"{len(hprobe.fwd)} probe steps"}
    step_gflop = BATCH * (STEP_GFLOP_PER_CLIP_FIXED + WAVLM_LAYER_GFLOP_PER_CLIP * layers)
    out = {
        "metric": "3s-clip train steps/sec (B=32, xattn fusion) at 1/2/4/8 MI355X",
        "value": round(world * args.steps / elapsed, 3),
        "unit": "steps/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 3),
        "ms_per_step_median": round(median_ms, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "bf16",
        "data": "synthetic (seeded 3 s clips resident in HBM; random-init weights; WavLM in train mode as in the "
                "reference: SpecAugment + dropout + LayerDrop)",
        "config": {"workload": ("ResNet18 + WavLM-base (frozen) + xattn fusion train step (fwd+bwd+Adam)"
                                if args.wavlm_unfreeze == 0 else
                                f"stage-2 fine-tuning step: WavLM last {args.wavlm_unfreeze} layers + ResNet18 layer4 + "
                                "xattn head trainable (fwd+bwd+Adam)"),
                   "per_gpu_batch": BATCH, "global_batch": BATCH * world, "frames": FRAMES, "image": SIZE,
                   "audio_samples": SAMPLES, "parallelism": f"dp{world}"},
        "clips_per_s": round(world * BATCH * args.steps / elapsed, 1),
        "final_loss": round(float(loss), 4) if loss is not None else None,
        "wavlm_layers_per_step": round(layers, 3),
        "step_tflop": round(step_gflop / 1e3, 4),
        "step_tflops_achieved": round(step_gflop / 1e3 / (median_ms * 1e-3), 1),
        "roofline": roof,
        "roofline_head": roof_head,
        "dp": dp,
        "peaks": peaks,
        "cpu_baseline": None,
    }
    if world == 1 and not args.no_cpu_baseline:
        threads = args.cpu_threads if args.cpu_threads > 0 else cpu_share_threads()
        out["cpu_baseline"] = cpu_baseline(threads, steps=args.cpu_steps, warmup=args.cpu_warmup)
    print(json.dumps(out), flush=True)
    if is_dist():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
