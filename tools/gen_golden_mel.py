"""Golden vectors of the mel audio path, from the imported REFERENCE (build container only).

Run:  python tools/gen_golden_mel.py   (needs /root/reference; never runs on the GPU box)

The reference's ``src/models/audio.py`` imports ``torchaudio.transforms`` and never uses it; torchaudio is absent, so
an empty stub module stands in for the import.  Weights come from ``oracle.params.init_tensor`` by state-dict name
(seed 0), waveforms from ``oracle.params.clip_inputs``, the log-mel input from the CPU restatement ``tests/mel_ref.py``
(fp32) -- so the tests regenerate weights and inputs without the reference.  Only seeds / shapes and the reference's
outputs are written to ``tests/golden``.
"""
from __future__ import annotations

import json
import sys
import types
from pathlib import Path

import numpy as np
import torch
from torch import nn

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
REF_SRC = Path("/root/reference/src")
sys.path.insert(0, str(REF_SRC))

for _name in ("torchaudio", "torchaudio.transforms"):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules["torchaudio"].transforms = sys.modules["torchaudio.transforms"]

from models.audio import AudioNet  # noqa: E402  (reference)
from models.fusion import FusionModel  # noqa: E402  (reference)

from oracle import params  # noqa: E402
from tests import mel_ref  # noqa: E402

OUT = ROOT / "tests" / "golden"
torch.set_num_threads(8)

B, ZERO_FROM = 3, 30000
FRAMES = (301, 37)  # T = 37 -> 18 -> 9 columns: the 16 adaptive-pool bins overlap
VIDEO_SEED, VIDEO_T = 77, 8


def mel_input() -> torch.Tensor:
    """[3, 1, 64, 301] fp32: log-mel of the oracle clips, the third silent from sample 30000 on."""
    wav = torch.from_numpy(params.clip_inputs(B, frames=1, size=1)[1]).clone()
    wav[2, :, ZERO_FROM:] = 0.0
    return mel_ref.log_mel(wav, 64, torch.float32)


class IdentityBackbone(nn.Module):
    def forward(self, x):
        return x


class StubVideo(nn.Module):
    """Feature-level stand-in for VideoNet (as in tools/gen_golden.py)."""

    def __init__(self, dim=512, num_classes=8):
        super().__init__()
        self.embedding_dim = dim
        self.backbone = IdentityBackbone()
        self.classifier = nn.Linear(dim, num_classes)

    def encode(self, x):
        return x

    def forward(self, x):
        return self.classifier(x)


def load_numpy_init(module: nn.Module, fix=None):
    new = {k: torch.from_numpy(params.init_tensor(k, tuple(v.shape), 0)) for k, v in module.state_dict().items()}
    if fix:
        fix(new)
    module.load_state_dict(new)


def video_feats():
    rng = np.random.Generator(np.random.PCG64(VIDEO_SEED))
    return (rng.standard_normal((B, VIDEO_T, 512)).astype(np.float32),
            rng.standard_normal((B, 512)).astype(np.float32))


def gen_audionet(use_resnet: bool, mel: torch.Tensor):
    m = AudioNet(num_classes=8, use_resnet=use_resnet, spec_augment=True).eval()
    load_numpy_init(m)
    out = {}
    with torch.no_grad():
        for T in FRAMES:
            x = mel[..., :T].contiguous()
            seq = m.encode_sequence(x)
            out[f"seq_{T}"], out[f"emb_{T}"], out[f"logits_{T}"] = seq.numpy(), m.encode(x).numpy(), m(x).numpy()
            if use_resnet:
                e = m.encoder
                stem = e.maxpool(e.relu(e.bn1(e.conv1(x))))
                out[f"stem_{T}"] = stem.numpy()
                out[f"layer4_{T}"] = e.layer4(e.layer3(e.layer2(e.layer1(stem)))).numpy()
    name = "audionet_resnet" if use_resnet else "audionet_cnn"
    np.savez_compressed(OUT / f"{name}.npz", zero_from=ZERO_FROM, **out)
    print(name, {k: (v.shape, float(np.abs(v).max())) for k, v in out.items()})
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


def gen_fusion(mel: torch.Tensor):
    v_seq, v_emb = video_feats()
    for name, mode, head in (("xattn_concat", "xattn", "concat"), ("xattn_gated", "xattn", "gated"),
                             ("late", "late", "concat"), ("concat", "concat", "concat"), ("gated", "gated", "concat")):
        audio = AudioNet(num_classes=8, use_resnet=False, spec_augment=True)
        m = FusionModel(audio, StubVideo(), num_classes=8, mode=mode, xattn_head=head, audio_n_mels=64).eval()

        def fix(sd):
            for k in ("xattn_gate.0.bias", "xattn_gate.3.bias", "gate.0.bias", "gate.3.bias"):
                if k in sd:
                    sd[k].fill_(-1.0)
        load_numpy_init(m, fix)
        with torch.no_grad():
            if mode == "xattn":
                out = m(torch.from_numpy(v_seq).view(B, VIDEO_T, 512, 1, 1), mel)
            else:
                out = m(torch.from_numpy(v_emb), mel)
        np.savez_compressed(OUT / f"fusion_mel_{name}.npz", out=out.numpy(), video_seed=VIDEO_SEED,
                            names=np.array(list(m.state_dict().keys())))
        print("fusion_mel", name, out[0, :3])


def main():
    mel = mel_input()
    keys = {"cnn": gen_audionet(False, mel), "resnet": gen_audionet(True, mel)}
    (OUT / "audionet_keys.json").write_text(json.dumps(keys, indent=0) + "\n")
    gen_fusion(mel)


if __name__ == "__main__":
    main()
