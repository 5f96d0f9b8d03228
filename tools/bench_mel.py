"""Time the mel audio path with HIP events (5 warm-up runs, the median of 20): ``clips.log_mel``, the forward of each
``AudioNet`` encoder, and ``TorchModelRunner.predict_probs`` of an xattn mel model fed waveforms beside the WavLM
runner in the same process -- at B = 64 clips of 48,000 samples -- plus the CPU ``torch.stft`` restatement of the front
end (tests/mel_ref.py) on 16 threads.  Writes profiles/mel/bench_mel.json and prints it.
    python tools/bench_mel.py [B]"""
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from multimodalemotionrecognition_amd.audio import AudioNet  # noqa: E402
from multimodalemotionrecognition_amd.clips import log_mel  # noqa: E402
from multimodalemotionrecognition_amd.optimized_runtime import TorchModelRunner  # noqa: E402
from multimodalemotionrecognition_amd.train import build_model  # noqa: E402
from tests import mel_ref  # noqa: E402

WARMUP, RUNS = 5, 20


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
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    S = 48000
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    wav_host = (0.1 * torch.randn(B, 1, S, generator=g)).clamp(-1, 1)
    wav = wav_host.to(dev)
    out = {"device": torch.cuda.get_device_name(0), "B": B, "S": S, "warmup": WARMUP, "runs": RUNS}

    ms = timed_ms(lambda: log_mel(wav))
    T = 1 + S // 160
    tiles = -(-T // 32)
    # per 32-step tile: 13 column tiles x 2 row tiles x 2 (cos, sin) x 100 K-steps + the mel product, 2 * 16 * 16 * 4 each
    flop = B * tiles * (13 * 2 * 2 * 100 + 8 * 52) * 2 * 16 * 16 * 4
    hbm = B * (S + 64 * T) * 4 + 2 * 400 * 208 * 4 + 208 * 64 * 4
    out["log_mel"] = {"ms": round(ms, 4), "clips_per_s": round(B / ms * 1e3, 1), "matrix_gflop": round(flop / 1e9, 2),
                      "fp32_mfma_bound_us_at_157TF": round(flop / 157e12 * 1e6, 1),
                      "hbm_mbytes": round(hbm / 1e6, 1), "hbm_bound_us_at_8TBps": round(hbm / 8e12 * 1e6, 1),
                      "x_mfma_bound": round(ms * 1e3 / (flop / 157e12 * 1e6), 1)}

    mel = log_mel(wav)
    for name, resnet in (("audiocnn", False), ("audioresnet18", True)):
        torch.manual_seed(0)
        m = AudioNet(num_classes=8, use_resnet=resnet).to(dev).eval()
        with torch.no_grad():
            t = timed_ms(lambda: m.encode_sequence(mel))
        out[f"{name}_encode_sequence"] = {"ms": round(t, 4), "clips_per_s": round(B / t * 1e3, 1)}

    g2 = torch.Generator().manual_seed(1)
    video = torch.randn(B, 8, 3, 112, 112, generator=g2).to(dev)
    for name, wavlm in (("mel_cnn", False), ("wavlm", True)):
        torch.manual_seed(0)
        src = build_model(8, "xattn", pretrained_video=False, use_wavlm=wavlm, use_resnet_audio=False)
        runner = TorchModelRunner(checkpoint={"model": src.state_dict()}, device=dev)
        del src
        t = wall_ms(lambda: runner.predict_probs(video, wav))
        out[f"predict_probs_xattn_{name}"] = {"ms": round(t, 3), "clips_per_s": round(B / t * 1e3, 1)}
        del runner
        torch.cuda.empty_cache()

    torch.set_num_threads(16)
    ts = []
    for i in range(WARMUP + RUNS):
        t0 = time.perf_counter()
        mel_ref.log_mel(wav_host, 64, torch.float32)
        if i >= WARMUP:
            ts.append((time.perf_counter() - t0) * 1e3)
    c = statistics.median(ts)
    out["cpu_torch_stft_16_threads"] = {"ms": round(c, 3), "clips_per_s": round(B / c * 1e3, 1)}

    d = ROOT / "profiles" / "mel"
    d.mkdir(parents=True, exist_ok=True)
    (d / "bench_mel.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
