"""Training of the mel audio path on the device (csrc/audionet_train.hip, audio.py).

A, B: the kernels against fp64 torch restatements on the CPU, under the project's rule (tests/kernel_parity.py): a
      kernel's error is at most 16x the error of the fp32 restatement, both from the same fp32 inputs.
C:    the whole model against the imported reference in float64 (tools/gen_golden_mel_train.py), bar 1e-4 of max-abs.
D, E: reproducibility, side effects, SpecAugment on the device.
F, G: the public training path, and what stays refused.

Every test prints the ratios it measures before asserting."""
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests.kernel_parity import EPS32, assert_fp64_parity
from tests.test_audionet_gpu import _StubVideo, load_numpy_init, mel_input

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLD = Path(__file__).resolve().parent / "golden"
LAYERS = ((1, 16, True), (16, 32, True), (32, 64, False))
EPS, MOMENTUM, BINS = 1e-5, 0.1, 16

# (name, shape, input scale, input offset, seed): A1 has partial tiles in both axes, an odd width dropped by the first
# pool and 9 < 16 columns at the adaptive pool; A2 is A1 in the log-mel range (the variance-cancellation case); A3 drops
# an odd height and width at both pools, takes layer 3's statistics over 3 values and pools from one column.
# The seeds were chosen on the CPU so that the fp64 restatement meets _assert_decided below.
CASES = {"A1": ((2, 1, 20, 37), 1.0, 0.0, 1), "A2": ((2, 1, 20, 37), 15.0, -40.0, 1), "A3": ((3, 1, 7, 5), 1.0, 0.0, 0)}
_CHAIN = {}


def chain_inputs(name):
    shape, scale, offset, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    P = {"x": torch.randn(shape, generator=g) * scale + offset}
    h, w = shape[2], shape[3]
    for i, (cin, cout, pool) in enumerate(LAYERS):
        P[f"w{i}"] = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
        P[f"b{i}"] = torch.randn(cout, generator=g) * 0.1
        P[f"gamma{i}"] = torch.randn(cout, generator=g)  # negative scales too
        P[f"beta{i}"] = torch.randn(cout, generator=g) * 0.3
        P[f"rm{i}"] = torch.randn(cout, generator=g) * 0.3
        P[f"rv{i}"] = torch.rand(cout, generator=g) * 1.5 + 0.5
        if pool:
            h, w = h // 2, w // 2
    P["gseq"] = torch.randn(shape[0], BINS, 64, generator=g)
    return P


def restate(P, dtype):
    """conv2d -> batch_norm(training) -> relu -> max_pool2d ... -> adaptive_avg_pool2d with autograd, in ``dtype``."""
    out, leaves, zs, acts, ys = {}, {}, [], [], []
    h = P["x"].to(dtype)
    for i, (_, _, pool) in enumerate(LAYERS):
        for k in ("w", "b", "gamma", "beta"):
            leaves[f"{k}{i}"] = P[f"{k}{i}"].to(dtype).requires_grad_()
        rm, rv = P[f"rm{i}"].to(dtype).clone(), P[f"rv{i}"].to(dtype).clone()
        z = F.conv2d(h, leaves[f"w{i}"], leaves[f"b{i}"], padding=1)
        z.retain_grad()
        a = F.batch_norm(z, rm, rv, leaves[f"gamma{i}"], leaves[f"beta{i}"], True, MOMENTUM, EPS)
        h = torch.relu(a)
        if pool:
            h = F.max_pool2d(h, 2)
        h.retain_grad()
        zs.append(z), acts.append(a), ys.append(h)
        out[f"rm{i}"], out[f"rv{i}"] = rm, rv
    seq = F.adaptive_avg_pool2d(h, (1, BINS)).squeeze(2).transpose(1, 2)
    (seq * P["gseq"].to(dtype)).sum().backward()
    out["seq"] = seq.detach()
    for i in range(3):
        out[f"y{i}"] = ys[i].detach()
        out[f"dw{i}"], out[f"db{i}"] = leaves[f"w{i}"].grad, leaves[f"b{i}"].grad
        out[f"dgamma{i}"], out[f"dbeta{i}"] = leaves[f"gamma{i}"].grad, leaves[f"beta{i}"].grad
        if i:
            out[f"dx{i}"] = ys[i - 1].grad
    return out, [a.detach() for a in acts], [z.grad for z in zs]


def _assert_decided(acts):
    """The condition on the inputs, on the fp64 restatement alone: an arg-max or ReLU flip would not be a kernel error
    but fails an element-wise comparison, so no pre-ReLU value lies within 1e-5 of zero and no pooling window with a
    positive maximum has its top two values closer than 1e-5."""
    for i, (_, _, pool) in enumerate(LAYERS):
        a = acts[i]
        assert float(a.abs().min()) >= 1e-5, (i, float(a.abs().min()))
        if pool:
            B, C, H, W = a.shape
            win = a[:, :, :H // 2 * 2, :W // 2 * 2].reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5)
            top = win.reshape(B, C, H // 2, W // 2, 4).sort(dim=-1, descending=True).values
            gap = (top[..., 0] - top[..., 1])[top[..., 0] > 0]
            assert gap.numel() == 0 or float(gap.min()) >= 1e-5, (i, float(gap.min()))


def chain_refs(name):
    """(inputs, fp64 results, fp32 results, max_c sum |dz64| per layer): computed once, shared, never modified."""
    if name not in _CHAIN:
        P = chain_inputs(name)
        r64, acts, dzs = restate(P, torch.float64)
        _assert_decided(acts)
        r32, _, _ = restate(P, torch.float32)
        _CHAIN[name] = (P, r64, r32, [float(dz.abs().sum(dim=(0, 2, 3)).max()) for dz in dzs])
    return _CHAIN[name]


@pytest.mark.parametrize("name", list(CASES))
def test_layer_chain_against_restatements(name):
    from multimodalemotionrecognition_amd import kernels as K

    P, r64, r32, dz_sums = chain_refs(name)
    d = {k: v.to(DEV) for k, v in P.items()}
    got, saved, h = {}, [], d["x"]
    for i, (cin, cout, pool) in enumerate(LAYERS):
        bn = nn.BatchNorm2d(cout, eps=EPS, momentum=MOMENTUM).to(DEV).train()
        with torch.no_grad():
            bn.weight.copy_(d[f"gamma{i}"]), bn.bias.copy_(d[f"beta{i}"])
            bn.running_mean.copy_(d[f"rm{i}"]), bn.running_var.copy_(d[f"rv{i}"])
        z = K.audiocnn_train_conv(h, d[f"w{i}"], d[f"b{i}"])
        ss = K.bn_train_stats(z, bn)
        saved.append((h, z, ss))
        h = K.bn_relu_pool_fwd(z, ss, pool)
        got[f"y{i}"], got[f"rm{i}"], got[f"rv{i}"] = h, bn.running_mean.clone(), bn.running_var.clone()
        assert int(bn.num_batches_tracked) == 1
    got["seq"] = K.adaptive_avgpool_seq(h, BINS)
    g = K.adaptive_avgpool_seq_bwd(d["gseq"], h.shape[2], h.shape[3])
    for i in (2, 1, 0):
        cin, cout, pool = LAYERS[i]
        hin, z, ss = saved[i]
        for k in ("dgamma", "dbeta", "db"):
            got[f"{k}{i}"] = torch.zeros(cout, device=DEV)
        got[f"dw{i}"] = torch.zeros(cout, cin, 3, 3, device=DEV)
        if i == 0:
            assert K.bn_relu_pool_bwd(z, ss, g, pool, got["dgamma0"], got["dbeta0"], got["db0"], x=hin,
                                      dw1=got["dw0"]) is None
        else:
            dz = K.bn_relu_pool_bwd(z, ss, g, pool, got[f"dgamma{i}"], got[f"dbeta{i}"], got[f"db{i}"])
            K.audiocnn_wgrad(hin, dz, got[f"dw{i}"])
            g = got[f"dx{i}"] = K.audiocnn_dgrad(dz, d[f"w{i}"])
    torch.cuda.synchronize()
    for k in sorted(r64):
        # the conv biases' true gradient is zero: the bar is the rounding any summation order may leave
        extra = 16 * EPS32 * dz_sums[int(k[-1])] if k.startswith("db") and not k.startswith("dbeta") else 0.0
        assert_fp64_parity(got[k], r64[k], r32[k], extra=extra, what=f"{name} {k}")


@pytest.mark.parametrize("H,W", [(5, 9), (16, 75), (1, 1)])
def test_adaptive_pool_backward(H, W):
    from multimodalemotionrecognition_amd import kernels as K

    g = torch.Generator().manual_seed(100 * H + W)
    gseq = torch.randn(2, BINS, 64, generator=g)
    refs = []
    for dt in (torch.float64, torch.float32):
        x = torch.zeros(2, 64, H, W, dtype=dt, requires_grad=True)
        (F.adaptive_avg_pool2d(x, (1, BINS)).squeeze(2).transpose(1, 2) * gseq.to(dt)).sum().backward()
        refs.append(x.grad)
    assert_fp64_parity(K.adaptive_avgpool_seq_bwd(gseq.to(DEV), H, W), refs[0], refs[1], what=f"pool bwd {H}x{W}")


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(5, 16, 32, 32, 150), (14, 32, 64, 16, 75)])
def test_weight_gradient_over_several_tiles_per_workgroup(B, Cin, Cout, H, W):
    """More 4 x 16 pixel tiles (400 / 280) than the launch has workgroups (256): each walks several and keeps its
    accumulators across them.  W is no multiple of 16, so the last tile column is partial."""
    from multimodalemotionrecognition_amd import kernels as K

    g = torch.Generator().manual_seed(Cin)
    x, dz = torch.randn(B, Cin, H, W, generator=g).relu(), torch.randn(B, Cout, H, W, generator=g)
    assert B * -(-H // 4) * -(-W // 16) > K.AUDIOCNN_WGRAD_WGS
    refs = []
    for dt in (torch.float64, torch.float32):
        w = torch.zeros(Cout, Cin, 3, 3, dtype=dt, requires_grad=True)
        (F.conv2d(x.to(dt), w, padding=1) * dz.to(dt)).sum().backward()
        refs.append(w.grad)
    dw = torch.zeros(Cout, Cin, 3, 3, device=DEV)
    K.audiocnn_wgrad(x.to(DEV), dz.to(DEV), dw)
    assert_fp64_parity(dw, refs[0], refs[1], what=f"wgrad {Cin}->{Cout} B={B}")


def _audionet(spec_augment=False):
    from multimodalemotionrecognition_amd.audio import AudioNet

    return load_numpy_init(AudioNet(num_classes=8, use_resnet=False, spec_augment=spec_augment)).to(DEV).train()


def _step(m, x, labels=(1, 5, 2)):
    """One forward + backward from zeroed gradients: (logits, loss, {name: grad})."""
    from multimodalemotionrecognition_amd.losses import CrossEntropyLoss

    m.zero_grad(set_to_none=True)
    logits = m(x)
    loss = CrossEntropyLoss()(logits, torch.tensor(labels, device=DEV))
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach().clone(), loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("T", [37, 301])
def test_model_against_reference(T):
    """Measured on an MI355X, error / max-abs of the golden: see DESIGN.md section 4h2 (the worst is the first
    conv's weight gradient at T = 301, 4e-6; fp32 torch on the CPU is 1.5e-4 off fp64 there)."""
    g = np.load(GOLD / "mel_train_cnn.npz")
    m = _audionet()
    logits, loss, grads = _step(m, mel_input()[..., :T].contiguous().to(DEV), tuple(int(v) for v in g["labels"]))
    got = {"logits": logits, "loss": loss}
    got.update({f"grad.{k}": v for k, v in grads.items()})
    got.update({f"buf.{k}": v for k, v in m.named_buffers()})
    bad = []
    for key in g.files:
        if not key.endswith(f"@{T}"):
            continue
        k = key[:-len(f"@{T}")]
        want = torch.from_numpy(g[key])
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(want) == 1
            continue
        scale = float(want.abs().max())
        if k.startswith("grad.encoder.features.") and k.endswith(".bias") and int(k.split(".")[3]) in (0, 4, 8):
            scale = float(np.abs(g[key.replace(".bias@", ".weight@")]).max())  # true value zero: the conv's dw scale
        ratio = float((got[k].detach().double().cpu() - want).abs().max()) / scale
        print(f"golden T={T} {k}: err / max-abs = {ratio:.3e}")
        assert bool(torch.isfinite(got[k]).all()), k
        if ratio > 1e-4:
            bad.append((k, ratio))
    assert not bad, bad


def test_reproducible_and_side_effects():
    x = mel_input()[..., :37].contiguous().to(DEV)
    m = _audionet()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    bns = [m.encoder.features[i] for i in (1, 5, 9)]
    r0 = [(b.running_mean.clone(), b.running_var.clone()) for b in bns]
    a = _step(m, x)
    r1 = [(b.running_mean.clone(), b.running_var.clone()) for b in bns]
    assert all(int(b.num_batches_tracked) == 1 for b in bns)
    m(x)
    assert all(int(b.num_batches_tracked) == 2 for b in bns)
    for b, (m0, v0), (m1, v1) in zip(bns, r0, r1):  # the same batch moves the statistics by the same rule twice
        assert not torch.equal(m0, m1) and not torch.equal(v0, v1)
        for s0, s1, s2 in ((m0, m1, b.running_mean), (v0, v1, b.running_var)):
            assert float(((s2 - 0.9 * s1) - (s1 - 0.9 * s0)).abs().max()) <= 1e-5 * float(s1.abs().max())
    m.load_state_dict(state)
    b = _step(m, x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    # frozen in train mode (stage 1), and under no_grad: batch statistics, moving running statistics, nothing saved
    for frozen in (True, False):
        m.load_state_dict(state)
        for p in m.parameters():
            p.requires_grad = not frozen
        if frozen:
            out = m(x)
        else:
            with torch.no_grad():
                out = m(x)
        assert out.grad_fn is None and not out.requires_grad and torch.equal(out, a[0])
        assert all(int(bn.num_batches_tracked) == 1 for bn in bns)
        assert all(torch.equal(bn.running_mean, r[0]) and torch.equal(bn.running_var, r[1]) for bn, r in zip(bns, r1))


def test_spec_augment_on_the_device():
    gold = np.load(GOLD / "spec_augment_draws.npz")
    applied = [s for s in range(gold["keep"].shape[0]) if not gold["keep"][s].all()]
    skipped = [s for s in range(gold["keep"].shape[0]) if gold["keep"][s].all()]
    x = mel_input().contiguous().to(DEV)  # [3, 1, 64, 301]
    x0 = x.clone()
    plain, aug = _audionet(False), _audionet(True)
    state = {k: v.clone() for k, v in plain.state_dict().items()}

    def run(m, inp, seed):
        m.load_state_dict(state)
        torch.manual_seed(seed)
        return _step(m, inp)

    keep = torch.from_numpy(gold["keep"][applied[0]]).to(DEV)
    want = run(plain, x.masked_fill(~keep, 0.0), applied[0])
    got = run(aug, x, applied[0])
    assert torch.equal(x, x0)  # the caller's tensor is left alone
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert all(torch.equal(got[2][k], want[2][k]) for k in want[2])
    clean = run(plain, x, skipped[0])
    assert not torch.equal(clean[0], want[0])
    got = run(aug, x, skipped[0])
    assert torch.equal(got[0], clean[0]) and all(torch.equal(got[2][k], clean[2][k]) for k in clean[2])
    # [B, n_mels, T] comes back with the channel dimension, as in the reference
    torch.manual_seed(applied[0])
    y = aug.spec_augment(x[:, 0])
    assert y.shape == x.shape and torch.equal(y, x.masked_fill(~keep, 0.0)) and torch.equal(x, x0)


def _log_mel_like(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 1, 64, T, generator=g) * 15.0 - 40.0).to(DEV)


def test_train_step_audio_mode():
    from multimodalemotionrecognition_amd.train import TrainStep, build_model, build_optimizer, make_loss

    x, labels = _log_mel_like(4, 37, 5), torch.tensor([0, 3, 5, 6], device=DEV)

    def run():
        torch.manual_seed(11)
        m = build_model(8, "audio", use_wavlm=False, use_resnet_audio=False).to(DEV)
        m.spec_augment.time_mask_param = 8  # T = 37: the default 40 can draw a mask as long as the clip
        step = TrainStep(m, build_optimizer(m), make_loss("audio"), "audio")
        losses = [step(None, x, labels)[0].clone() for _ in range(8)]
        torch.cuda.synchronize()
        return losses, {k: v.clone() for k, v in m.state_dict().items()}

    la, sa = run()
    print("audio-mode losses", [float(v) for v in la])
    assert all(bool(torch.isfinite(v)) for v in la) and float(la[-1]) < float(la[0])
    lb, sb = run()
    assert all(torch.equal(p, q) for p, q in zip(la, lb)) and all(torch.equal(sa[k], sb[k]) for k in sa)


def _xattn_model():
    from multimodalemotionrecognition_amd.audio import AudioNet
    from multimodalemotionrecognition_amd.fusion import FusionModel

    torch.manual_seed(7)
    return FusionModel(AudioNet(num_classes=8, use_resnet=False), _StubVideo(), num_classes=8, mode="xattn",
                       audio_n_mels=64).to(DEV)


def _xattn_batch():
    g = torch.Generator().manual_seed(9)
    return (torch.randn(4, 8, 512, 1, 1, generator=g).to(DEV), _log_mel_like(4, 301, 6),
            torch.tensor([1, 2, 4, 7], device=DEV))


@pytest.mark.parametrize("fused", [True, False])
def test_train_step_xattn_mode(fused, monkeypatch):
    """The audio encoder runs on FusionModel's side stream, and autograd runs its backward there."""
    from multimodalemotionrecognition_amd import xattn_fused
    from multimodalemotionrecognition_amd.train import TrainStep, build_optimizer, make_loss

    monkeypatch.setattr(xattn_fused, "ENABLED", fused)
    m = _xattn_model()
    loss, _ = TrainStep(m, build_optimizer(m), make_loss("xattn"), "xattn")(*_xattn_batch())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    for k, p in m.audio_model.encoder.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.ne(0).any()), k
    assert all(int(m.audio_model.encoder.features[i].num_batches_tracked) == 1 for i in (1, 5, 9))


@pytest.mark.parametrize("stage", [1, 2])
def test_two_stage_freeze_policy(stage):
    from multimodalemotionrecognition_amd.train import (TrainStep, apply_two_stage_freeze_policy,
                                                        build_fusion_stage_optimizer, make_loss)

    m = _xattn_model()
    apply_two_stage_freeze_policy(m, stage=stage, unfreeze_audio=True)
    before = m.audio_model.encoder.features[0].weight.detach().clone()
    loss, _ = TrainStep(m, build_fusion_stage_optimizer(m, stage), make_loss("xattn"), "xattn")(*_xattn_batch())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    assert all(int(m.audio_model.encoder.features[i].num_batches_tracked) == 1 for i in (1, 5, 9))
    assert torch.equal(before, m.audio_model.encoder.features[0].weight) == (stage == 1)


def test_refusals():
    from multimodalemotionrecognition_amd.audio import AudioCNN, AudioNet

    m = AudioNet(num_classes=8, use_resnet=True).to(DEV).train()
    x = torch.zeros(2, 1, 64, 37, device=DEV)
    for fn in (m, m.encode, m.encode_sequence, m.encoder.forward_sequence):
        with pytest.raises(NotImplementedError, match="AudioResNet18"):
            fn(x)
    enc = AudioCNN().to(DEV).train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):  # 1 x 1 x 1 at layer 3, as torch refuses
        enc.pooled_features(torch.zeros(1, 1, 4, 4, device=DEV))
    assert all(int(enc.features[i].num_batches_tracked) == 0 for i in (1, 5, 9))  # refused before any launch
