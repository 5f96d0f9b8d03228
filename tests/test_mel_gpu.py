"""Device log-mel front end (csrc/mel.hip, clips.log_mel) against the fp64 CPU restatement tests/mel_ref.py.

Bars: the kernel's error may be at most 16 x the error of the fp32 ``torch.stft`` restatement on the same inputs (a
direct 400-term sum against an FFT's ~9 stages: sqrt(400 / 9) ~ 6.7 in random-walk error, doubled).  Inputs: four rows
of S = 4000 samples (T = 26: the second 16-step row tile is partial) and S = 201 (T = 2, the shortest input)."""
import numpy as np
import pytest
import torch

from tests import mel_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = [(4000, 64), (4000, 40), (201, 64), (201, 40)]
_REF = {}


def _ref(S, n_mels):
    """(inputs, mel64, mel32) of the CPU restatement, computed once per case."""
    key = (S, n_mels)
    if key not in _REF:
        x = mel_ref.frontend_inputs(S)
        _REF[key] = (x, mel_ref.mel_power(x, n_mels, torch.float64), mel_ref.mel_power(x, n_mels, torch.float32))
    return _REF[key]


@pytest.mark.parametrize("S,n_mels", CASES)
def test_mel_power_against_fp64(S, n_mels):
    from multimodalemotionrecognition_amd.clips import log_mel

    x, m64, m32 = _ref(S, n_mels)
    got = log_mel(x.to(DEV).unsqueeze(1), n_mels=n_mels, to_db=False)
    assert got.shape == (4, 1, n_mels, 1 + S // 160) and got.dtype == torch.float32
    assert torch.equal(got, log_mel(x.to(DEV), n_mels=n_mels, to_db=False))  # [B, S] form
    err, bar = mel_ref.power_error(got.cpu(), m64), mel_ref.power_error(m32, m64)
    print("power error", S, n_mels, "kernel", err.tolist(), "restatement", bar.tolist(), "ratio", (err / bar).tolist())
    assert torch.all(err <= 16.0 * bar)
    # all-zero frames (the tone row's tail) are exactly zero power
    if S == 4000:
        assert not got[1, 0, :, -5:].any()


@pytest.mark.parametrize("S,n_mels", CASES)
def test_log_mel_db_against_fp64(S, n_mels):
    from multimodalemotionrecognition_amd.clips import log_mel

    x, m64, m32 = _ref(S, n_mels)
    got = log_mel(x.to(DEV).unsqueeze(1), n_mels=n_mels).cpu()
    d64 = mel_ref.to_db(m64)
    err = (got.double() - d64).abs()[[0, 2]].amax()
    bar = (mel_ref.to_db(m32).double() - d64).abs()[[0, 2]].amax()
    print("dB error (noise rows)", S, n_mels, "kernel", float(err), "restatement", float(bar))
    assert float(err) <= 16.0 * float(bar)
    if S == 4000:  # all-zero frames: 10 * log10(1e-10) as fp32 torch gives it, within 4 ulp at 100
        floor = 10.0 * torch.log10(torch.tensor(1e-10, dtype=torch.float32))
        assert float((got[1, 0, :, -5:] - floor).abs().max()) <= 4 * 2.0 ** -17


def test_two_runs_are_bit_identical():
    from multimodalemotionrecognition_amd.clips import log_mel

    x = _ref(4000, 64)[0].to(DEV)
    a, b = log_mel(x), log_mel(x)
    assert torch.equal(a, b)
    # a row's result does not depend on its batch neighbours or on the row stride
    wide = torch.zeros(4, 4100, device=DEV)
    wide[:, :4000] = x
    assert torch.equal(log_mel(wide[:, :4000]), a)
    assert torch.equal(log_mel(x[2:3]), a[2:3])


def test_full_clip_shape_and_more_time_tiles():
    """A 3 s clip: T = 301 = nine 32-step tiles and a 13-step one; n_mels = 128 and 1 are the limits."""
    from multimodalemotionrecognition_amd.clips import log_mel

    g = torch.Generator().manual_seed(5)
    x = 0.1 * torch.randn(2, 1, 48000, generator=g)
    for n_mels in (64, 128, 1):
        got = log_mel(x.to(DEV), n_mels=n_mels, to_db=False)
        assert got.shape == (2, 1, n_mels, 301)
        m64, m32 = mel_ref.mel_power(x, n_mels, torch.float64), mel_ref.mel_power(x, n_mels, torch.float32)
        err, bar = mel_ref.power_error(got.cpu(), m64), mel_ref.power_error(m32, m64)
        print("power error 48000", n_mels, err.tolist(), bar.tolist())
        assert torch.all(err <= 16.0 * bar)


def test_argument_errors():
    from multimodalemotionrecognition_amd.clips import log_mel

    with pytest.raises(ValueError):
        log_mel(torch.zeros(2, 1, 200, device=DEV))
    with pytest.raises(ValueError):
        log_mel(torch.zeros(2, 1, 4000, device=DEV), win_length=320)
    with pytest.raises(ValueError):
        log_mel(torch.zeros(2, 1, 4000, device=DEV), n_mels=0)


@pytest.fixture(scope="module")
def items(tmp_path_factory):
    from oracle import io_ref as R

    d = tmp_path_factory.mktemp("melclips")
    rng = np.random.default_rng(41)
    out = []
    for i in range(5):
        fp = d / f"f{i}.npy"
        np.save(fp, rng.integers(0, 256, (9, 96, 100, 3), dtype=np.uint8))
        wp = d / f"a{i}.wav"
        R.write_wav(wp, rng.uniform(-0.5, 0.5, (int(16000 * (2.2 + 0.3 * i)), 1)), 16000, "pcm16")
        out.append((str(fp), str(wp), int(rng.integers(0, 8)), None, {"actor": f"{i:02d}"}))
    return out


def test_clip_loader_mel_batches(items):
    from multimodalemotionrecognition_amd.clips import log_mel
    from multimodalemotionrecognition_amd.data import ClipLoader

    wav = list(ClipLoader(items, batch_size=2, workers=2, drop_last=False))
    mel = list(ClipLoader(items, batch_size=2, workers=2, drop_last=False, audio_features="mel"))
    assert len(wav) == len(mel) == 3
    for (v0, a0, y0, _), (v1, a1, y1, _) in zip(wav, mel):
        assert a1.shape == (a0.shape[0], 1, 64, 301) and a0.shape[1:] == (1, 48000)
        assert torch.equal(a1, log_mel(a0)) and torch.equal(v0, v1) and torch.equal(y0, y1)
    m40 = next(iter(ClipLoader(items, batch_size=2, workers=2, audio_features="mel", n_mels=40)))[1]
    assert torch.equal(m40, log_mel(wav[0][1], n_mels=40))
    with pytest.raises(ValueError):
        ClipLoader(items, audio_features="mfcc")
