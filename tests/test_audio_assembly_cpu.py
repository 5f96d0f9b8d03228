"""Device audio clip assembly, the parts that need no device: the augmentation draws against ``load_audio_wav``'s
sequence restated here, the host slicing rule against the host resampler, and the refusals that come before any
device work."""
import numpy as np
import pytest
import torch

from multimodalemotionrecognition_amd import clips
from multimodalemotionrecognition_amd import data as D


def _host_draws(rng, target, n_noise):
    """The draws of data.load_audio_wav (ravdess.py:519-576) in its order: (level, snr_db or None, start or None)."""
    level = rng.uniform(0.0, 1.0)
    if level < 0.5:
        return level, None, None
    snr_db = float(rng.choice([20.0, 15.0, 10.0])) if level < 0.9 else 5.0
    if not n_noise:
        return level, snr_db, None
    tiled = n_noise if n_noise >= target else n_noise * (target // n_noise + 1)
    max_start = max(0, tiled - target)
    start = int(rng.integers(0, max_start + 1)) if max_start > 0 else 0
    return level, snr_db, start


@pytest.mark.parametrize("target,n_noise", [(48000, 160000), (48000, 333), (48000, 48000), (1000, 1000), (1000, 0)])
def test_draw_audio_augment_reproduces_the_host_sequence(target, n_noise):
    seen = set()
    for seed in range(32):
        a, b = np.random.default_rng([seed, 3, 7]), np.random.default_rng([seed, 3, 7])
        level, snr, start = _host_draws(a, target, n_noise)
        mode, dstart, dsnr, dseed = clips.draw_audio_augment(b, target, n_noise)
        print("draw", seed, target, n_noise, "host", level, snr, start, "device", mode, dstart, dsnr, dseed)
        if snr is None:
            assert (mode, dstart, dsnr, dseed) == (0, 0, 0.0, 0)
        elif n_noise:
            assert (mode, dstart, dsnr, dseed) == (1, start, snr, 0)
            tiled = n_noise if n_noise >= target else n_noise * (target // n_noise + 1)
            assert 0 <= dstart <= max(0, tiled - target)
            if tiled == target:
                assert dstart == 0  # max_start == 0: no integers() draw
        else:
            assert mode == 2 and dstart == 0 and dsnr == snr and 0 <= dseed < 2 ** 63
            a.integers(0, 2 ** 63 - 1)  # the one extra draw stands where the host's rng.normal does
        assert a.bit_generator.state == b.bit_generator.state  # both generators consumed the same draws
        seen.add((mode, dsnr))
    assert {m for m, _ in seen} == ({0, 1} if n_noise else {0, 2})
    assert {s for m, s in seen if m} == {20.0, 15.0, 10.0, 5.0}


@pytest.mark.parametrize("target", [1, 1000, 48000])
@pytest.mark.parametrize("sr_in", [48000, 44100, 8000, 16000])
def test_resample_needed_inputs_keeps_the_first_outputs(sr_in, target):
    up, down = clips.resample_ratio(sr_in, 16000)
    need = clips.resample_needed_inputs(target, up, down)
    n = need + 5000
    rng = np.random.default_rng(sr_in + target)
    x = (rng.normal(0, 0.3, n) + 0.2 * np.sin(2 * np.pi * 440.0 * np.arange(n) / sr_in)).astype(np.float32)
    whole = D.resample(x, sr_in, 16000)
    sliced = D.resample(x[:need], sr_in, 16000)
    print("needed inputs", sr_in, target, "->", need, "outputs of the slice", sliced.size, "of the whole", whole.size)
    assert whole.size >= target and sliced.size >= target
    assert np.array_equal(sliced[:target], whole[:target])
    if sr_in != 16000:  # the rule is tight: one sample fewer changes a kept output (the newest input of the last one)
        half = 10 * max(up, down)
        assert need == ((target - 1) * down + half) // up + 1
    else:
        assert need == target
    assert clips.resample_needed_inputs(0, up, down) == 0


def test_refusals_come_before_any_device_work(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("device work after a bad argument")

    monkeypatch.setattr(clips.K, "LIB", no_launch)
    monkeypatch.setattr(clips, "_h2d", no_launch)
    x = torch.zeros(100)
    for bad in (0, -16000):
        with pytest.raises(ValueError, match="positive"):
            clips.resample_clips(x, bad, 16000, device="cuda")
        with pytest.raises(ValueError, match="positive"):
            clips.resample_clips(x, 48000, bad, device="cuda")
        with pytest.raises(ValueError, match="positive"):
            clips.assemble_waveforms([x], [bad], device="cuda")
    # 3.2 MHz -> 16 kHz is 1 / 200: kmax = 4001 and a block's span 255 * 200 + 1 + 4001 floats, past the LDS limit
    up, down = clips.resample_ratio(3200000, 16000)
    kmax = 2 * 10 * max(up, down) // up + 1
    assert 255 * down // up + 1 + kmax > clips.RESAMPLE_MAX_SPAN
    with pytest.raises(ValueError, match="stages at most"):
        clips.resample_clips(x, 3200000, 16000, device="cuda")
    with pytest.raises(ValueError, match="stages at most"):
        clips.assemble_waveforms([x, x], [16000, 3200000], device="cuda")
    with pytest.raises(RuntimeError, match="MI355X"):
        clips.resample_clips(x, 48000, 16000)  # host clips and no device named
    with pytest.raises(ValueError, match="equal output count"):
        clips.resample_clips([x, torch.zeros(50)], 48000, 16000, device="cuda")
    with pytest.raises(RuntimeError, match="MI355X"):
        clips.mix_noise_clips(torch.zeros(2, 10), [(0, 0, 0.0, 0)] * 2)


def test_library_refuses_bad_scalars_before_any_launch():
    from multimodalemotionrecognition_amd._lib import LIB

    LIB.load()
    f = LIB._fns
    fake = 1 << 20  # never dereferenced: every call below fails its checks first
    # mer_resample_clips(B, target, up, down, kmax, table, packed, offsets, lengths, out, stream)
    ok = [2, 1000, 1, 3, 61, fake, fake, fake, fake, fake, None]
    assert f["mer_resample_clips"](0, *ok[1:]) == 0 and f["mer_resample_clips"](2, 0, *ok[2:]) == 0
    for pos, bad in ((1, -1), (2, 0), (3, 0), (4, 60), (5, None), (6, None), (7, None), (8, None), (9, None),
                     (0, 65536)):
        args = list(ok)
        args[pos] = bad
        assert f["mer_resample_clips"](*args) == 1, pos
    assert f["mer_resample_clips"](1, 1000, 1, 200, 4001, fake, fake, fake, fake, fake, None) == 1  # span > 12288
    # mer_mix_noise_clips(B, target, wav, mode, start, snr_db, seed, noise, n_noise, ztable, parts, scale, out, stream)
    ok = [2, 1000, fake, fake, fake, fake, fake, fake, 333, fake, fake, fake, fake, None]
    assert f["mer_mix_noise_clips"](0, *ok[1:]) == 0
    for pos, bad in ((1, -1), (2, None), (3, None), (4, None), (5, None), (6, None), (7, None), (8, -1), (9, None),
                     (10, None), (11, None), (12, None), (0, 65536)):
        args = list(ok)
        args[pos] = bad
        assert f["mer_mix_noise_clips"](*args) == 1, pos


def test_mix_descriptors_are_validated_on_the_host(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("device work after a bad descriptor")

    monkeypatch.setattr(clips.K, "LIB", no_launch)
    monkeypatch.setattr(clips, "_h2d", no_launch)
    wav = torch.zeros(1, 10)
    for bad in [(3, 0, 10.0, 0), (1, 0, 10.0, 0), (2, -1, 10.0, 0), (2, 0, float("nan"), 0), (2, 0, 10.0, 2 ** 63),
                (2, 0, 10.0, -1)]:
        with pytest.raises(ValueError):
            clips.mix_noise_clips(wav, [bad])
    with pytest.raises(ValueError, match="draws for"):
        clips.mix_noise_clips(wav, [])


def test_device_audio_loader_refuses_the_cpu():
    with pytest.raises(RuntimeError, match="runs on the MI355X"):
        D.ClipLoader([], device="cpu", device_audio=True)
    assert D.ClipLoader([], device="cpu").device_audio is False  # the default is the host path
