"""Golden vectors of the mel audio path in TRAINING mode, from the imported REFERENCE (build container only).

Run:  python tools/gen_golden_mel_train.py   (needs /root/reference; never runs on the GPU box)

As tools/gen_golden_mel.py: an empty torchaudio stub stands in for the reference's unused import, weights come from
``oracle.params.init_tensor`` by state-dict name (seed 0) and the log-mel input from ``tests/mel_ref.py``, so the tests
regenerate both without the reference.  Only the reference's outputs are written to ``tests/golden``:

* ``mel_train_cnn.npz``: ``AudioNet(8, use_resnet=False, spec_augment=False).train()`` in float64 on the fp32 goldens'
  input at T = 37 and 301, labels (1, 5, 2), ``F.cross_entropy``: logits, loss, every parameter gradient and the
  BatchNorm buffers after the one forward.  The same in fp32 is printed against it (relative to each tensor's max-abs).
* ``spec_augment_draws.npz``: the reference's ``SpecAugment(20, 40, p=0.5).train()`` under seeds 0..15 on
  ones(2, 1, 64, 301) -- the keep-mask and the ``torch.rand(1)`` drawn right after it -- and, on T = 37 under seeds
  0..39, which seeds raise.
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, "/root/reference/src")

for _name in ("torchaudio", "torchaudio.transforms"):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules["torchaudio"].transforms = sys.modules["torchaudio.transforms"]

from models.audio import AudioNet, SpecAugment  # noqa: E402  (reference)

from oracle import params  # noqa: E402
from tests import mel_ref  # noqa: E402

OUT = ROOT / "tests" / "golden"
torch.set_num_threads(8)

B, FRAMES, LABELS = 3, (37, 301), (1, 5, 2)
DRAW_SEEDS, RAISE_SEEDS = 16, 40


def mel_input() -> torch.Tensor:
    wav = torch.from_numpy(params.clip_inputs(B, frames=1, size=1)[1]).clone()
    wav[2, :, int(np.load(OUT / "audionet_cnn.npz")["zero_from"]):] = 0.0
    return mel_ref.log_mel(wav, 64, torch.float32)


def run(dtype, x):
    m = AudioNet(num_classes=8, use_resnet=False, spec_augment=False)
    m.load_state_dict({k: torch.from_numpy(params.init_tensor(k, tuple(v.shape), 0)) for k, v in m.state_dict().items()})
    m = m.to(dtype).train()
    logits = m(x.to(dtype))
    loss = F.cross_entropy(logits, torch.tensor(LABELS))
    loss.backward()
    out = {"logits": logits.detach(), "loss": loss.detach()}
    out.update({f"grad.{k}": p.grad for k, p in m.named_parameters()})
    out.update({f"buf.{k}": v for k, v in m.named_buffers()})
    return out


def gen_train(mel):
    out = {}
    for T in FRAMES:
        x = mel[..., :T].contiguous()
        r64, r32 = run(torch.float64, x), run(torch.float32, x)
        for k, v in r64.items():
            out[f"{k}@{T}"] = v.numpy()
            if v.dtype == torch.float64:
                err = float((r32[k].double() - v).abs().max() / v.abs().max().clamp_min(1e-300))
                print(f"fp32 vs fp64  T={T:3d} {k:40s} max|.|={float(v.abs().max()):.3e}  err/max={err:.2e}")
    np.savez_compressed(OUT / "mel_train_cnn.npz", labels=np.array(LABELS), **out)


def gen_draws():
    masks, nxt, applied = [], [], 0
    for seed in range(DRAW_SEEDS):
        torch.manual_seed(seed)
        y = SpecAugment(20, 40, p=0.5).train()(torch.ones(2, 1, 64, 301))
        nxt.append(float(torch.rand(1)))
        assert torch.equal(y[0], y[1])
        masks.append(y[0, 0].numpy() != 0)
        applied += int(not masks[-1].all())
    raises = []
    for seed in range(RAISE_SEEDS):
        torch.manual_seed(seed)
        try:
            SpecAugment(20, 40, p=0.5).train()(torch.ones(2, 1, 64, 37))
        except RuntimeError:
            raises.append(seed)
    print("draws: applied", applied, "of", DRAW_SEEDS, "; raising at T = 37:", raises)
    assert applied >= 4 and DRAW_SEEDS - applied >= 4 and len(raises) >= 1
    np.savez_compressed(OUT / "spec_augment_draws.npz", keep=np.stack(masks), next_rand=np.array(nxt, np.float64),
                        raises_37=np.array(raises, np.int64))


if __name__ == "__main__":
    gen_train(mel_input())
    gen_draws()
