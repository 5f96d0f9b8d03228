"""The reference's mel-spectrogram audio model (``src/models/audio.py``) on the MI355X kernels.

``AudioNet`` is what the reference's ``train.py`` builds unless ``--use_wavlm`` is passed: ``AudioCNN`` by default
(``AudioNet(use_resnet=False)``), ``AudioResNet18`` with ``--use_resnet_audio``.  Constructor arguments and
attribute names are the reference's, so its checkpoints load unchanged (25 state-dict keys for the CNN model, 124 for
the ResNet one).

* ``AudioCNN`` runs in eval mode on ``csrc/audionet.hip`` (fp32): three fused conv + BatchNorm + ReLU (+ MaxPool)
  launches, the adaptive pool + transpose, and ``proj`` on the fp32 GEMM.
* ``AudioResNet18`` runs in eval mode on the frame trunk's bf16 kernels (``csrc/conv.hip``, ``csrc/bn_pool.hip``):
  NHWC bf16 activations, one implicit-GEMM conv + eval BatchNorm apply per layer, then the adaptive pool from that
  layout and ``fc`` in fp32.
* ``AudioCNN`` trains on ``csrc/audionet_train.hip`` (fp32): per layer the conv output ``z`` is stored, its batch
  statistics are merged from per-plane (mean, M2) records (Chan's formula, fixed order) and update the running
  statistics, and the backward recomputes the arg-max / ReLU mask from ``z``.  One
  ``torch.autograd.Function`` covers ``pooled_features``; gradients land in ``fusion.grad_buffer`` of each parameter.
  A frozen encoder in train mode still normalises with batch statistics and moves the running ones, but saves nothing.
* ``SpecAugment`` draws on the host with the reference's calls in the reference's order (``draw``) and masks a copy on
  the device: unlike the reference it never writes into the caller's tensor.
* Training of ``AudioResNet18`` is not built: every training-mode forward of it raises ``NotImplementedError``.  So does
  a training-mode forward of any mel model on a host tensor (the path runs on the device kernels only).

Input: the log-mel spectrogram ``[B, 1, n_mels, T]`` fp32 of ``clips.log_mel`` (``RavdessAVDataset``'s audio item,
ravdess.py:607).
"""
from __future__ import annotations

import torch
from torch import nn

from . import kernels as K
from .nn_ops import hip_linear
from .temporal import TemporalPooler, _MeanPoolFn

_TRAIN_MSG = ("training of the mel audio path over AudioResNet18 is not built (batch-statistics BatchNorm and backward on "
              "the bf16 trunk kernels): call .eval(); the trainable audio models are AudioCNN (use_resnet=False) and WavLM")
_HOST_TRAIN_MSG = ("training of the mel audio path on a host tensor is not built: it runs on the device kernels; "
                   "move the input to the GPU")


def _check_mel(x: torch.Tensor) -> torch.Tensor:
    if x.dim() != 4 or x.shape[1] != 1:
        raise ValueError(f"the mel audio model takes log-mel spectrograms [B, 1, n_mels, T], got {tuple(x.shape)}")
    if not x.is_cuda:
        raise RuntimeError("the mel audio model runs on the MI355X kernels; move the input to the GPU")
    return x.contiguous().float()


class SpecAugment(nn.Module):
    """audio.py:10-52.  An identity in eval mode.  In training mode the draws are the reference's, made on the host
    from torch's global generator (``draw``); the bands then travel to one device kernel as arguments.

    Unlike the reference, which zeroes the bands in the caller's tensor in place, this returns a masked COPY and
    leaves the caller's tensor alone (the first conv and its weight gradient read the same data).  When nothing is
    drawn the input itself is returned, as in the reference."""

    def __init__(self, freq_mask_param: int = 20, time_mask_param: int = 40, num_masks: int = 2, p: float = 0.5):
        super().__init__()
        self.freq_mask_param = freq_mask_param
        self.time_mask_param = time_mask_param
        self.num_masks = num_masks
        self.p = p

    def draw(self, n_mels: int, time_steps: int):
        """The host part of a training-mode call (audio.py:26-50), needing no device: ``None`` when the call leaves
        its input alone, else ``(freq_bands, time_bands)``, lists of ``(start, length)``.  The calls, their order and
        so the number of values taken from the generator are the reference's; where the reference fails
        (``torch.randint`` with an empty range, a mask as long as the axis) this fails with the same torch error."""
        if self.num_masks > K.SPEC_AUGMENT_MAX_BANDS:
            raise ValueError(f"SpecAugment: num_masks <= {K.SPEC_AUGMENT_MAX_BANDS} (the bands are kernel arguments), "
                             f"got {self.num_masks}")
        if torch.rand(1).item() > self.p:
            return None
        freq_bands, time_bands = [], []
        for _ in range(self.num_masks):
            if self.freq_mask_param > 0:
                freq_mask_len = torch.randint(0, self.freq_mask_param + 1, (1,)).item()
                if freq_mask_len > 0:
                    freq_bands.append((torch.randint(0, n_mels - freq_mask_len, (1,)).item(), freq_mask_len))
            if self.time_mask_param > 0:
                time_mask_len = torch.randint(0, self.time_mask_param + 1, (1,)).item()
                if time_mask_len > 0:
                    time_bands.append((torch.randint(0, time_steps - time_mask_len, (1,)).item(), time_mask_len))
        return freq_bands, time_bands

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: [B, 1, n_mels, T] or [B, n_mels, T]; a masked call returns [B, 1, n_mels, T]."""
        if not self.training:
            return x
        if not x.is_cuda:
            raise NotImplementedError(_HOST_TRAIN_MSG)
        if x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[1] != 1):
            raise ValueError(f"SpecAugment takes [B, 1, n_mels, T] or [B, n_mels, T], got {tuple(x.shape)}")
        bands = self.draw(x.shape[-2], x.shape[-1])
        if bands is None:
            return x
        y = K.spec_augment_mask(x.detach().contiguous().float(), *bands)
        return y if y.dim() == 4 else y.unsqueeze(1)


class _AudioCNNTrainFn(torch.autograd.Function):
    """``AudioCNN.pooled_features`` in training mode: the three conv + batch-statistics BatchNorm + ReLU (+ MaxPool)
    layers and the adaptive pool.  ``params`` are ``features``' parameters (autograd's view of them; the kernels read
    the modules' tensors); ``save`` keeps (layer input, z, scale / shift / mean / invstd) per layer for the backward."""

    LAYERS = ((0, 1, True), (4, 5, True), (8, 9, False))

    @staticmethod
    def forward(ctx, x, enc, save, *params):
        saved, h = [], x
        for ci, bi, pool in _AudioCNNTrainFn.LAYERS:
            conv, bn = enc.features[ci], enc.features[bi]
            z = K.audiocnn_train_conv(h, conv.weight, conv.bias)
            ss = K.bn_train_stats(z, bn)
            if save:
                saved.append((h, z, ss))
            h = K.bn_relu_pool_fwd(z, ss, pool)
        ctx.saved, ctx.enc, ctx.hw = saved, enc, tuple(h.shape[2:])
        return K.adaptive_avgpool_seq(h, enc.temporal_bins)

    @staticmethod
    def backward(ctx, gseq):
        from .fusion import grad_buffer

        enc, grads = ctx.enc, {}

        def buf(p):
            if p is None or not p.requires_grad:
                return None
            grads[id(p)] = grad_buffer(p)
            return grads[id(p)]

        mods = [(enc.features[ci], enc.features[bi], pool) for ci, bi, pool in _AudioCNNTrainFn.LAYERS]
        lowest = min(i for i, (conv, bn, _) in enumerate(mods)
                     if any(p.requires_grad for p in (*conv.parameters(), *bn.parameters())))
        g = K.adaptive_avgpool_seq_bwd(gseq.contiguous().float(), *ctx.hw)
        for i in (2, 1, 0):
            if i < lowest:  # nothing below needs a gradient: the input never does
                break
            (h, z, ss), (conv, bn, pool) = ctx.saved[i], mods[i]
            dgamma, dbeta, dbias, dw = buf(bn.weight), buf(bn.bias), buf(conv.bias), buf(conv.weight)
            if i == 0 and dw is not None:  # dz of layer 1 is never stored
                K.bn_relu_pool_bwd(z, ss, g, pool, dgamma, dbeta, dbias, x=h, dw1=dw)
                break
            dz = K.bn_relu_pool_bwd(z, ss, g, pool, dgamma, dbeta, dbias)
            if i > 0 and dw is not None:
                K.audiocnn_wgrad(h, dz, dw)
            if i > lowest:
                g = K.audiocnn_dgrad(dz, conv.weight)
        return (None, None, None, *[grads.get(id(p)) for p in enc.features.parameters()])


class AudioResNet18(nn.Module):
    """audio.py:55-119 in eval mode, bf16.  NOT torchvision's topology: no residual connections; a layer is an
    optional 1x1 / stride-s conv + BN (no ReLU) followed by two conv-BN-ReLU-conv-BN blocks; the stem is 7x7 /
    stride 2 on one channel."""

    def __init__(self, embedding_dim: int = 128, temporal_bins: int = 16) -> None:
        super().__init__()
        self.embedding_dim = embedding_dim
        self.temporal_bins = temporal_bins
        self.conv1 = nn.Conv2d(1, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, 64, 2, stride=1)
        self.layer2 = self._make_layer(64, 128, 2, stride=2)
        self.layer3 = self._make_layer(128, 256, 2, stride=2)
        self.layer4 = self._make_layer(256, 512, 2, stride=2)
        self.sequence_pool = nn.AdaptiveAvgPool2d((1, temporal_bins))
        self.fc = nn.Linear(512, embedding_dim)

    def _make_layer(self, in_channels: int, out_channels: int, blocks: int, stride: int = 1) -> nn.Sequential:
        layers = []
        if stride != 1 or in_channels != out_channels:
            layers.append(nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=stride, bias=False),
                                        nn.BatchNorm2d(out_channels)))
        for _ in range(blocks):
            layers.append(self._make_block(out_channels, out_channels))
        return nn.Sequential(*layers)

    def _make_block(self, in_channels: int, out_channels: int) -> nn.Module:
        return nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size=3, padding=1, bias=False),
                             nn.BatchNorm2d(out_channels), nn.ReLU(inplace=True),
                             nn.Conv2d(out_channels, out_channels, kernel_size=3, padding=1, bias=False),
                             nn.BatchNorm2d(out_channels))

    @staticmethod
    def _conv_bn(x: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, relu: bool) -> torch.Tensor:
        """NHWC bf16 ``x`` -> [relu](bn(conv(x))) in the same layout: the weight packed from the live parameter,
        the trunk's implicit-GEMM conv without statistics, BatchNorm on the running statistics."""
        Kc, C, R, S = conv.weight.shape
        stride, pad = conv.stride[0], conv.padding[0]
        N, H, W, Cp = x.shape
        if C > Cp or conv.stride[0] != conv.stride[1] or conv.padding[0] != conv.padding[1] or conv.bias is not None:
            raise ValueError(f"unsupported conv {conv} on an input of {Cp} channels")
        wp = torch.empty(Kc, R * S * Cp, device=x.device, dtype=torch.bfloat16)
        K.pack_conv_weight(conv.weight.detach().float().contiguous(), wp, Cp, False)
        Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
        y = torch.empty(N, Ho, Wo, Kc, device=x.device, dtype=torch.bfloat16)
        K.conv_fwd(x, wp, y, None, R, S, stride, pad)
        ms = torch.empty(Kc, 2, device=x.device, dtype=torch.float32)
        K.bn_finalize(None, N * Ho * Wo, bn.eps, 0.0, ms, bn.running_mean, bn.running_var)
        out = torch.empty_like(y)
        K.bn_apply(y, ms, bn.weight, bn.bias, out, relu=relu)
        return out

    def forward_features(self, x: torch.Tensor):
        """[B, 1, n_mels, T] -> (stem + maxpool output, layer4 output), both NHWC bf16."""
        if self.training:
            raise NotImplementedError(_TRAIN_MSG)
        x = _check_mel(x)
        B, _, H, W = x.shape
        with torch.no_grad():
            x8 = torch.empty(B, H, W, 8, device=x.device, dtype=torch.bfloat16)
            K.pack_input_nhwc(x, x8)
            a = self._conv_bn(x8, self.conv1, self.bn1, relu=True)
            Hp, Wp = (a.shape[1] - 1) // 2 + 1, (a.shape[2] - 1) // 2 + 1
            stem = torch.empty(B, Hp, Wp, a.shape[-1], device=x.device, dtype=torch.bfloat16)
            K.maxpool_fwd(a, stem, torch.empty(stem.shape, device=x.device, dtype=torch.uint8))
            h = stem
            for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
                for m in layer:
                    if len(m) == 2:  # the downsample pair: conv + BN, no ReLU
                        h = self._conv_bn(h, m[0], m[1], relu=False)
                    else:  # conv-BN-ReLU-conv-BN
                        h = self._conv_bn(self._conv_bn(h, m[0], m[1], relu=True), m[3], m[4], relu=False)
        return stem, h

    def forward_sequence(self, x: torch.Tensor) -> torch.Tensor:
        _, feat = self.forward_features(x)
        with torch.no_grad():
            pooled = K.adaptive_avgpool_seq_nhwc(feat, self.temporal_bins)
        return hip_linear(pooled, self.fc)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _MeanPoolFn.apply(self.forward_sequence(x))  # seq.mean(dim=1)


class AudioCNN(nn.Module):
    """audio.py:122-154, fp32: eval mode on csrc/audionet.hip, training mode on csrc/audionet_train.hip."""

    def __init__(self, embedding_dim: int = 128, temporal_bins: int = 16) -> None:
        super().__init__()
        self.temporal_bins = temporal_bins
        self.features = nn.Sequential(
            nn.Conv2d(1, 16, kernel_size=3, padding=1), nn.BatchNorm2d(16), nn.ReLU(inplace=True), nn.MaxPool2d(2),
            nn.Conv2d(16, 32, kernel_size=3, padding=1), nn.BatchNorm2d(32), nn.ReLU(inplace=True), nn.MaxPool2d(2),
            nn.Conv2d(32, 64, kernel_size=3, padding=1), nn.BatchNorm2d(64), nn.ReLU(inplace=True))
        self.proj = nn.Sequential(nn.Linear(64, embedding_dim), nn.ReLU(inplace=True))
        self.sequence_pool = nn.AdaptiveAvgPool2d((1, temporal_bins))
        self.embedding_dim = embedding_dim

    def pooled_features(self, x: torch.Tensor) -> torch.Tensor:
        """``features`` + ``sequence_pool`` + transpose: [B, 1, n_mels, T] -> [B, temporal_bins, 64]."""
        if self.training and not x.is_cuda:
            raise NotImplementedError(_HOST_TRAIN_MSG)
        x = _check_mel(x)
        if x.shape[2] < 4 or x.shape[3] < 4:
            raise ValueError(f"AudioCNN pools twice by 2: the spectrogram must be at least 4 x 4, got {tuple(x.shape)}")
        if self.training:
            if x.shape[0] * (x.shape[2] // 4) * (x.shape[3] // 4) < 2:  # before any launch, as torch's batch_norm
                raise ValueError("Expected more than 1 value per channel when training, got input size "
                                 f"{[x.shape[0], 64, x.shape[2] // 4, x.shape[3] // 4]}")
            params = list(self.features.parameters())
            save = torch.is_grad_enabled() and any(p.requires_grad for p in params)
            return _AudioCNNTrainFn.apply(x.detach(), self, save, *params)
        with torch.no_grad():
            for ci, bi, pool in ((0, 1, True), (4, 5, True), (8, 9, False)):
                x = K.audiocnn_conv(x, self.features[ci], self.features[bi], pool)
            return K.adaptive_avgpool_seq(x, self.temporal_bins)

    def forward_sequence(self, x: torch.Tensor) -> torch.Tensor:
        return hip_linear(self.pooled_features(x), self.proj[0], act="relu")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _MeanPoolFn.apply(self.forward_sequence(x))  # seq.mean(dim=1)


class AudioNet(nn.Module):
    """audio.py:157-206."""

    def __init__(self, num_classes: int, embedding_dim: int = 128, use_resnet: bool = True, spec_augment: bool = True,
                 temporal_pooling: str = "mean", temporal_num_heads: int = 4, temporal_num_layers: int = 1,
                 temporal_dropout: float = 0.1) -> None:
        super().__init__()
        self.embedding_dim = embedding_dim
        self.sequence_dim = embedding_dim
        self.encoder = AudioResNet18(embedding_dim=embedding_dim) if use_resnet else AudioCNN(embedding_dim=embedding_dim)
        self.temporal_pool = TemporalPooler(dim=embedding_dim, mode=temporal_pooling, num_heads=temporal_num_heads,
                                            num_layers=temporal_num_layers, dropout=temporal_dropout)
        self.spec_augment = SpecAugment(freq_mask_param=20, time_mask_param=40, p=0.5) if spec_augment else None
        self.classifier = nn.Linear(embedding_dim, num_classes)

    def encode_sequence(self, x: torch.Tensor) -> torch.Tensor:
        """Encoder states for the fusion models: [B, 16, embedding_dim] fp32."""
        if self.training:
            if isinstance(self.encoder, AudioResNet18):
                raise NotImplementedError(_TRAIN_MSG)
            if not x.is_cuda:  # before any draw
                raise NotImplementedError(_HOST_TRAIN_MSG)
            if self.spec_augment is not None:
                x = self.spec_augment(x)
        return self.encoder.forward_sequence(x)

    def encode(self, x: torch.Tensor) -> torch.Tensor:
        return self.temporal_pool(self.encode_sequence(x))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return hip_linear(self.encode(x), self.classifier)
