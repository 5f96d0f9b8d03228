"""The reference's mel-spectrogram audio model (``src/models/audio.py``) for inference on the MI355X kernels.

``AudioNet`` is what the reference's ``train.py`` builds unless ``--use_wavlm`` is passed: ``AudioCNN`` by default
(``AudioNet(use_resnet=False)``), ``AudioResNet18`` with ``--use_resnet_audio``.  Constructor arguments and
attribute names are the reference's, so its checkpoints load unchanged (25 state-dict keys for the CNN model, 124 for
the ResNet one).

* ``AudioCNN`` runs in eval mode on ``csrc/audionet.hip`` (fp32): three fused conv + BatchNorm + ReLU (+ MaxPool)
  launches, the adaptive pool + transpose, and ``proj`` on the fp32 GEMM.
* ``AudioResNet18`` runs in eval mode on the frame trunk's bf16 kernels (``csrc/conv.hip``, ``csrc/bn_pool.hip``):
  NHWC bf16 activations, one implicit-GEMM conv + eval BatchNorm apply per layer, then the adaptive pool from that
  layout and ``fc`` in fp32.
* Training of the mel path (SpecAugment draws, batch-statistics BatchNorm, backward) is not built: every forward in
  training mode raises ``NotImplementedError``.

Input: the log-mel spectrogram ``[B, 1, n_mels, T]`` fp32 of ``clips.log_mel`` (``RavdessAVDataset``'s audio item,
ravdess.py:607).
"""
from __future__ import annotations

import torch
from torch import nn

from . import kernels as K
from .nn_ops import hip_linear
from .temporal import TemporalPooler, _MeanPoolFn

_TRAIN_MSG = ("training of the mel audio path is not built (SpecAugment draws, batch-statistics BatchNorm, backward): "
              "call .eval(); the trainable audio path is WavLM")


def _check_mel(x: torch.Tensor) -> torch.Tensor:
    if x.dim() != 4 or x.shape[1] != 1:
        raise ValueError(f"the mel audio model takes log-mel spectrograms [B, 1, n_mels, T], got {tuple(x.shape)}")
    if not x.is_cuda:
        raise RuntimeError("the mel audio model runs on the MI355X kernels; move the input to the GPU")
    return x.contiguous().float()


class SpecAugment(nn.Module):
    """audio.py:10-52.  An identity in eval mode; the training-mode draws are not built."""

    def __init__(self, freq_mask_param: int = 20, time_mask_param: int = 40, num_masks: int = 2, p: float = 0.5):
        super().__init__()
        self.freq_mask_param = freq_mask_param
        self.time_mask_param = time_mask_param
        self.num_masks = num_masks
        self.p = p

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.training:
            raise NotImplementedError(_TRAIN_MSG)
        return x


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
    """audio.py:122-154 in eval mode, fp32."""

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
        if self.training:
            raise NotImplementedError(_TRAIN_MSG)
        x = _check_mel(x)
        if x.shape[2] < 4 or x.shape[3] < 4:
            raise ValueError(f"AudioCNN pools twice by 2: the spectrogram must be at least 4 x 4, got {tuple(x.shape)}")
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
            raise NotImplementedError(_TRAIN_MSG)
        return self.encoder.forward_sequence(x)

    def encode(self, x: torch.Tensor) -> torch.Tensor:
        return self.temporal_pool(self.encode_sequence(x))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return hip_linear(self.encode(x), self.classifier)
