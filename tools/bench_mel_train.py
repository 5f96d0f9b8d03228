"""Time the training of the mel audio path with HIP events (5 warm-up runs, the median of 20), in one process, at
B = 32 and 64 clips of T = 301 frames:

* the training-mode ``AudioNet`` (AudioCNN) forward + backward on csrc/audionet_train.hip;
* its eval forward, for scale;
* the same network as plain ``torch.nn`` modules in fp32 train mode on the same device (forward + backward) -- the
  only alternative a user has;
* the encoder's passes one by one (the kernels.py wrappers in the order ``audio._AudioCNNTrainFn`` calls them), with
  the bytes each pass has to move.

Writes profiles/mel/bench_mel_train.json and prints it.
    python tools/bench_mel_train.py"""
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F
from torch import nn

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from multimodalemotionrecognition_amd import kernels as K  # noqa: E402
from multimodalemotionrecognition_amd.audio import AudioNet  # noqa: E402
from multimodalemotionrecognition_amd.losses import CrossEntropyLoss  # noqa: E402

WARMUP, RUNS, T = 5, 20, 301
DEV = "cuda"


def timed_ms(fn):
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


class TorchAudioNet(nn.Module):
    """AudioNet(use_resnet=False, temporal_pooling="mean") from stock modules."""

    def __init__(self):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(1, 16, 3, padding=1), nn.BatchNorm2d(16), nn.ReLU(inplace=True), nn.MaxPool2d(2),
            nn.Conv2d(16, 32, 3, padding=1), nn.BatchNorm2d(32), nn.ReLU(inplace=True), nn.MaxPool2d(2),
            nn.Conv2d(32, 64, 3, padding=1), nn.BatchNorm2d(64), nn.ReLU(inplace=True))
        self.pool = nn.AdaptiveAvgPool2d((1, 16))
        self.proj = nn.Sequential(nn.Linear(64, 128), nn.ReLU(inplace=True))
        self.classifier = nn.Linear(128, 8)

    def forward(self, x):
        seq = self.proj(self.pool(self.features(x)).squeeze(2).transpose(1, 2).contiguous())
        return self.classifier(seq.mean(dim=1))


def passes(m, x, gseq):
    """(name, fn, bytes) of every encoder pass, layer by layer; the tensors come from one real forward / backward."""
    enc, out, saved, h = m.encoder, [], [], x
    mb = lambda *ts: sum(t.numel() * 4 for t in ts)  # noqa: E731
    for i, (ci, bi, pool) in enumerate(((0, 1, True), (4, 5, True), (8, 9, False)), 1):
        conv, bn = enc.features[ci], enc.features[bi]
        z = K.audiocnn_train_conv(h, conv.weight, conv.bias)
        ss = K.bn_train_stats(z, bn)
        y = K.bn_relu_pool_fwd(z, ss, pool)
        out.append((f"L{i} conv -> z", lambda h=h, c=conv: K.audiocnn_train_conv(h, c.weight, c.bias), mb(h, z)))
        out.append((f"L{i} statistics", lambda z=z, b=bn: K.bn_train_stats(z, b), mb(z)))
        out.append((f"L{i} bn relu pool", lambda z=z, s=ss, p=pool: K.bn_relu_pool_fwd(z, s, p), mb(z, y)))
        saved.append((h, z, ss, conv, pool))
        h = y
    out.append(("adaptive pool", lambda h=h: K.adaptive_avgpool_seq(h, 16), mb(h)))
    g = K.adaptive_avgpool_seq_bwd(gseq, h.shape[2], h.shape[3])
    out.append(("adaptive pool bwd", lambda h=h: K.adaptive_avgpool_seq_bwd(gseq, h.shape[2], h.shape[3]), mb(g)))
    for i in (3, 2, 1):
        hin, z, ss, conv, pool = saved[i - 1]
        C = z.shape[1]
        dg, dbt, db = (torch.zeros(C, device=DEV) for _ in range(3))
        dw = torch.zeros_like(conv.weight)
        if i == 1:
            out.append(("L1 bn bwd + wgrad (no dz)", lambda z=z, s=ss, g=g, p=pool, hin=hin, a=(dg, dbt, db), dw=dw:
                        K.bn_relu_pool_bwd(z, s, g, p, *a, x=hin, dw1=dw), mb(z, z, g, hin)))
            break
        dz = K.bn_relu_pool_bwd(z, ss, g, pool, dg, dbt, db)
        out.append((f"L{i} bn bwd -> dz", lambda z=z, s=ss, g=g, p=pool, a=(dg, dbt, db):
                    K.bn_relu_pool_bwd(z, s, g, p, *a), mb(z, z, g, dz)))
        rows = K.audiocnn_wgrad_rows(z.shape[0], z.shape[2], z.shape[3], C)
        out.append((f"L{i} wgrad", lambda hin=hin, dz=dz, dw=dw: K.audiocnn_wgrad(hin, dz, dw),
                    mb(hin, dz) + 2 * rows * dw.numel() * 4))
        g = K.audiocnn_dgrad(dz, conv.weight)
        out.append((f"L{i} dgrad", lambda dz=dz, c=conv: K.audiocnn_dgrad(dz, c.weight), mb(dz, g)))
    return out


def main():
    out = {"device": torch.cuda.get_device_name(0), "T": T, "warmup": WARMUP, "runs": RUNS,
           "launches_per_step_encoder": {"forward": 15, "backward": 22}}
    for B in (32, 64):
        g = torch.Generator().manual_seed(0)
        x = (torch.randn(B, 1, 64, T, generator=g) * 15.0 - 40.0).to(DEV)
        labels = torch.randint(0, 8, (B,), generator=g).to(DEV)
        torch.manual_seed(0)
        m = AudioNet(num_classes=8, use_resnet=False, spec_augment=False).to(DEV)
        ref = TorchAudioNet().to(DEV).train()
        ce = CrossEntropyLoss()

        def ours():
            m.zero_grad(set_to_none=True)
            ce(m(x), labels).backward()

        def stock():
            ref.zero_grad(set_to_none=True)
            F.cross_entropy(ref(x), labels).backward()

        r = {}
        m.train()
        r["train_fwd_bwd_ms"] = round(timed_ms(ours), 4)
        with torch.no_grad():
            r["train_fwd_only_ms"] = round(timed_ms(lambda: m(x)), 4)
            m.eval()
            r["eval_fwd_ms"] = round(timed_ms(lambda: m(x)), 4)
        m.train()
        r["torch_nn_fwd_bwd_ms"] = round(timed_ms(stock), 4)
        r["speedup_over_torch_nn"] = round(r["torch_nn_fwd_bwd_ms"] / r["train_fwd_bwd_ms"], 3)
        r["target_met"] = r["train_fwd_bwd_ms"] <= r["torch_nn_fwd_bwd_ms"]
        with torch.no_grad():
            gseq = torch.randn(B, 16, 64, device=DEV)
            r["passes"] = [{"pass": n, "us": round(timed_ms(fn) * 1e3, 1), "mbytes": round(nb / 1e6, 1)}
                           for n, fn, nb in passes(m, x, gseq)]
        out[f"B{B}"] = r
        del m, ref
        torch.cuda.empty_cache()
    d = ROOT / "profiles" / "mel"
    d.mkdir(parents=True, exist_ok=True)
    (d / "bench_mel_train.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
