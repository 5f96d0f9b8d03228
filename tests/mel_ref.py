"""CPU restatement of the log-mel front end (ravdess.py:478-485) for the mel tests and goldens:
``torchaudio.transforms.MelSpectrogram(sample_rate=16000, n_mels, win_length=400, hop_length=160)`` followed by
``AmplitudeToDB()``, written with ``torch.stft`` and the ``torchaudio.functional.melscale_fbanks`` formula, in a chosen
dtype (fp32: what the reference computes; fp64: the yardstick).  torchaudio itself is absent, so parity against it
is unpinned; this file follows its documented definition."""
from __future__ import annotations

import math

import torch

N_FFT, HOP, SR = 400, 160, 16000


def melscale_fbanks(n_mels: int, dtype, sample_rate: int = SR, n_freqs: int = N_FFT // 2 + 1) -> torch.Tensor:
    """[n_freqs, n_mels]: HTK scale, f_min 0, f_max sr / 2, norm None."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=dtype)
    m_min = 2595.0 * math.log10(1.0 + 0.0 / 700.0)
    m_max = 2595.0 * math.log10(1.0 + (sample_rate / 2.0) / 700.0)
    m_pts = torch.linspace(m_min, m_max, n_mels + 2, dtype=dtype)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.max(torch.zeros(1, dtype=dtype), torch.min(down, up))


def mel_power(wav: torch.Tensor, n_mels: int = 64, dtype=torch.float32) -> torch.Tensor:
    """wav [B, S] or [B, 1, S] -> mel power [B, 1, n_mels, 1 + S // 160] in ``dtype`` (the MelSpectrogram output)."""
    if wav.dim() == 3:
        wav = wav[:, 0]
    x = wav.to(dtype)
    win = torch.hann_window(N_FFT, periodic=True, dtype=dtype)
    spec = torch.stft(x, N_FFT, hop_length=HOP, win_length=N_FFT, window=win, center=True, pad_mode="reflect",
                      normalized=False, onesided=True, return_complex=True)
    power = spec.real ** 2 + spec.imag ** 2  # [B, 201, T]
    mel = torch.matmul(power.transpose(-1, -2), melscale_fbanks(n_mels, dtype)).transpose(-1, -2)
    return mel.unsqueeze(1)


def to_db(mel: torch.Tensor) -> torch.Tensor:
    """AmplitudeToDB(): stype power, ref 1, amin 1e-10, no top_db."""
    return 10.0 * torch.log10(torch.clamp(mel, min=1e-10))


def log_mel(wav: torch.Tensor, n_mels: int = 64, dtype=torch.float32) -> torch.Tensor:
    return to_db(mel_power(wav, n_mels, dtype))


def frontend_inputs(S: int = 4000) -> torch.Tensor:
    """The four front-end test rows [4, S]: N(0, 0.1^2) noise; a 440 Hz tone for 2500 samples, then zeros;
    N(0, 0.8^2) noise clipped to +-1; a single impulse."""
    g = torch.Generator().manual_seed(1234)
    x = torch.zeros(4, S)
    x[0] = 0.1 * torch.randn(S, generator=g)
    n = min(2500, S)
    x[1, :n] = 0.5 * torch.sin(2.0 * math.pi * 440.0 * torch.arange(n, dtype=torch.float64) / SR).float()
    x[2] = (0.8 * torch.randn(S, generator=g)).clamp(-1.0, 1.0)
    x[3, S // 3] = 1.0
    return x


def power_error(mel: torch.Tensor, mel64: torch.Tensor) -> torch.Tensor:
    """Per input row: max over frames with a non-zero sum of max_bins |mel - mel64| / sum_bins mel64."""
    mel, mel64 = mel.double()[:, 0], mel64.double()[:, 0]
    tot = mel64.sum(dim=1)  # [B, T]
    err = (mel - mel64).abs().amax(dim=1)
    ratio = torch.where(tot > 0, err / tot.clamp_min(1e-300), torch.zeros_like(err))
    return ratio.amax(dim=1)
