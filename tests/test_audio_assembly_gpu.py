"""Device audio clip assembly (csrc/audio_clips.hip, clips.assemble_waveforms, ClipLoader(device_audio=True)).

Bars.  Bit-exact means ``torch.equal``.  R1 pins the batched resampler to ``clips.ResampleStream`` bit for bit (both
call one device function); R2 is tests/test_streaming_gpu.py's derived bound against scipy's float64
``resample_poly``: a K-term fp32 sum of products, one fmaf per tap, taps rounded to fp32 once, errs by at most
``(K + 2) * 2^-24 * sum |h_k| |x_k|``.  The mix's scale is within one fp32 ulp of its float64 restatement and, given
the device's own scale, the output is bit-exact; against the host ``data.mix_noise`` it lies within ``2^-22``: one ulp
of scale moves ``noise * scale`` by at most ``2^-23`` relative, values are clamped to [-1, 1], and the two roundings
add half an ulp each."""
import math

import numpy as np
import pytest
import torch

import test_timeline_gpu as TL  # its recording and its runners (built once per process, shared with that file)
from multimodalemotionrecognition_amd import clips
from multimodalemotionrecognition_amd import data as D
from oracle import io_ref as R
from tests import kernel_parity as KP

pytestmark = pytest.mark.gpu

DEV = "cuda"
SR = 16000
RATES = [48000, 44100, 8000, 16000]
LENGTHS = [0, 1, 29, 1000, 4001]
CAP = 8192  # a ring that holds every output of the longest clip: (4001 + 41) * 2 at 8 kHz
_CACHE = {}


def _signal(kind, sr_in, n, seed=0):
    if kind == "noise":
        g = torch.Generator().manual_seed(sr_in + 7 * n + seed)
        return torch.randn(n, generator=g) * 0.3
    return (0.5 * torch.sin(2 * math.pi * 440.0 * torch.arange(n, dtype=torch.float64) / sr_in)).float()


def _kmax(sr_in):
    up, down = clips.resample_ratio(sr_in, SR)
    return 0 if up == down else 2 * 10 * max(up, down) // up + 1


def _stream(sr_in, x, cap):
    """The clip through a fresh ResampleStream, then kmax zeros: (ring on the host, outputs emitted)."""
    ring = torch.zeros(cap, device=DEV)
    rs = clips.ResampleStream(sr_in, ring)
    rs.push(x)
    rs.push(torch.zeros(_kmax(sr_in)))
    assert rs.n_out <= cap
    return ring.cpu(), rs.n_out


def _clips(sr_in, kind):
    """The five ragged clips of one rate and the stream's outputs for each, computed once and left unchanged."""
    key = (sr_in, kind)
    if key not in _CACHE:
        xs = [_signal(kind, sr_in, n) for n in LENGTHS]
        _CACHE[key] = (xs, [_stream(sr_in, x, CAP) for x in xs])
    return _CACHE[key]


def _nout(n, sr_in):
    up, down = clips.resample_ratio(sr_in, SR)
    return clips.resample_outputs(n, up, down)


# ------------------------------------------------------------------------------------------------ resampler
@pytest.mark.parametrize("kind", ["noise", "tone"])
@pytest.mark.parametrize("sr_in", RATES)
def test_r1_same_bits_as_the_stream(sr_in, kind):
    xs, streams = _clips(sr_in, kind)
    offsets = np.cumsum([0] + LENGTHS[:-1])
    assert any(o % 4 for o in offsets)  # clips that do not start on a 16-byte boundary
    for target in (700, 2000):
        got = clips.resample_clips(xs, sr_in, SR, target, device=DEV).cpu()
        assert tuple(got.shape) == (len(xs), target)
        for b, (x, (ring, emitted)) in enumerate(zip(xs, streams)):
            keep = min(_nout(x.numel(), sr_in), target)
            assert emitted >= keep  # the stream fed kmax zeros has emitted every output the clip has
            same = torch.equal(got[b, :keep], ring[:keep])
            pad = float(got[b, keep:].abs().max()) if keep < target else 0.0
            print("R1", sr_in, kind, "target", target, "len", x.numel(), "kept", keep, "equal", same, "pad max", pad)
            assert same and pad == 0.0
        assert float(got[3].abs().max()) > 0.1  # a signal, not silence
    if sr_in == SR:  # equal rates: a copy / crop
        assert torch.equal(got[3, :1000], xs[3]) and torch.equal(got[4], xs[4][:2000])


@pytest.mark.parametrize("kind", ["noise", "tone"])
@pytest.mark.parametrize("sr_in", [48000, 44100, 8000])
def test_r2_fp64_bound(sr_in, kind):
    from scipy.signal import firwin, resample_poly

    xs, _ = _clips(sr_in, kind)
    up, down = clips.resample_ratio(sr_in, SR)
    half = 10 * max(up, down)
    h = firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0))
    target = 2000
    got = clips.resample_clips(xs, sr_in, SR, target, device=DEV).cpu().double().numpy()
    for b, x in enumerate(xs):
        if not x.numel():
            assert not got[b].any()
            continue
        ref = resample_poly(x.double().numpy(), up, down)
        assert ref.shape[0] == _nout(x.numel(), sr_in)
        keep = min(ref.shape[0], target)
        mag = resample_poly(x.double().abs().numpy(), up, down, window=np.abs(h))[:keep]  # sum |h_k| |x_k| per output
        p = (np.arange(keep) * down + half) % up
        K = (2 * half - p) // up + 1  # taps output o sums
        err = np.abs(got[b, :keep] - ref[:keep])
        bound = (K + 2) * 2.0 ** -24 * mag
        print("R2", sr_in, kind, "len", x.numel(), "kept", keep, "max err", err.max(), "max err / bound",
              float((err / np.maximum(bound, 1e-30)).max()))
        assert bool((err <= bound).all())
    assert float(np.abs(got[4]).max()) > 0.1


@pytest.mark.parametrize("sr_in", RATES)
def test_r3_isolation(sr_in):
    xs, _ = _clips(sr_in, "noise")
    target = 2000
    want = clips.resample_clips(xs, sr_in, SR, target, device=DEV)
    # a NaN-filled buffer (kernel_parity.padded_input's way): NaN in front of the first clip, in a gap after every
    # clip and behind the last; only the clips' own samples are numbers
    front, gap = 5, 3
    offsets, pos = [], front
    for n in LENGTHS:
        offsets.append(pos)
        pos += n + gap
    host = torch.full((pos + 4,), float("nan"))
    for o, x in zip(offsets, xs):
        host[o:o + x.numel()] = x
    assert any(o % 4 for o in offsets) and int(torch.isnan(host).sum()) == host.numel() - sum(LENGTHS)
    packed = host.to(DEV)
    g = KP.guarded_flat((len(xs), target), DEV)
    assert g.view.is_contiguous()
    g.view.fill_(float("nan"))
    clips.resample_packed(packed, offsets, LENGTHS, sr_in, SR, target, out=g.view)
    g.check(f"resample_clips {sr_in}")
    got = g.view
    nans = int(torch.isnan(got).sum())
    print("R3", sr_in, "NaN outputs", nans, "equal to the un-gapped run", torch.equal(got, want))
    assert nans == 0  # nothing outside a clip was read, and every element of the view was written
    assert torch.equal(got, want)


@pytest.mark.parametrize("sr_in", RATES)
def test_r4_determinism_and_batch_independence(sr_in):
    xs, _ = _clips(sr_in, "noise")
    for target in (700, 2000):
        a = clips.resample_clips(xs, sr_in, SR, target, device=DEV)
        b = clips.resample_clips(xs, sr_in, SR, target, device=DEV)
        ones = torch.cat([clips.resample_clips([x], sr_in, SR, target, device=DEV) for x in xs])
        print("R4", sr_in, target, "twice", torch.equal(a, b), "B=1 launches", torch.equal(a, ones))
        assert torch.equal(a, b) and torch.equal(a, ones)


def test_r5_long_input():
    n = 3_000_000
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, generator=g) * 0.3
    got = clips.resample_clips(x, 48000, SR, device=DEV)
    assert tuple(got.shape) == (1, 1_000_000)
    ring, emitted = _stream(48000, x, 1_000_064)
    assert emitted >= 1_000_000
    pos = torch.from_numpy(np.random.default_rng(5).integers(0, 1_000_000, 64))
    got = got[0].cpu()
    eq = [torch.equal(got[:300], ring[:300]), torch.equal(got[-300:], ring[999_700:1_000_000]),
          torch.equal(got[pos], ring[pos])]
    print("R5 first / last 300 and 64 positions equal the stream's:", eq, "max", float(got.abs().max()))
    assert all(eq) and float(got[pos].abs().max()) > 0.1


# ------------------------------------------------------------------------------------------------ mix
SNRS = [20.0, 15.0, 10.0, 5.0]


def _mix_rows(target=1000):
    g = torch.Generator().manual_seed(31)
    wav = torch.randn(6, target, generator=g) * 0.3
    wav[1] *= 2.5  # loud enough for the clamp to bite
    wav[4] = 0.0  # a silent clip
    wav[5, ::7] = 1.5  # a row left alone that overshoots [-1, 1] (a resampled clip may)
    wav[5, 3::11] = -1.25
    return wav


def _tracks():
    g = torch.Generator().manual_seed(32)
    return {"long": torch.randn(2500, generator=g) * 0.2, "tiled": torch.randn(333, generator=g) * 0.2,
            "silent": torch.zeros(400)}


def _restate_scale(w, v, snr_db):
    """float64: ps, pn means, scale = sqrt(ps / max(10^(snr / 10), 1e-8) / pn), 1 when pn <= 1e-8."""
    ps, pn = float(np.mean(w.astype(np.float64) ** 2)), float(np.mean(v.astype(np.float64) ** 2))
    want = ps / max(10.0 ** (snr_db / 10.0), 1e-8)
    return math.sqrt(want / pn) if pn > 1e-8 else 1.0


def _ulp_close(got, want64):
    w = np.float32(want64)
    return np.nextafter(w, np.float32(-np.inf)) <= np.float32(got) <= np.nextafter(w, np.float32(np.inf))


@pytest.mark.parametrize("track,starts", [("long", [0, 1499, 2000, 2499, 7]), ("tiled", [0, 332, 100, 5, 331]),
                                          ("silent", [0, 1, 2, 3, 399])])
def test_m1_mix_against_its_restatement(track, starts):
    target = 1000
    wav, noise = _mix_rows(target), _tracks()[track]
    n = noise.numel()
    assert track != "long" or (n > target and starts[2] + target > n)  # a window that wraps the track's end
    params = [(1, starts[b], SNRS[b], 0) for b in range(4)] + [(1, starts[4], 10.0, 0), (0, 0, 0.0, 0)]
    out, scale = clips.mix_noise_clips(wav.to(DEV), params, noise.to(DEV), return_scale=True)
    out3 = clips.mix_noise_clips(wav.to(DEV)[:, None, :], params, noise.to(DEV))
    assert tuple(out3.shape) == (6, 1, target) and torch.equal(out3[:, 0], out)
    out, scale = out.cpu().numpy(), scale.cpu().numpy()
    w, nz = wav.numpy(), noise.numpy()
    for b in range(5):
        v = nz[(starts[b] + np.arange(target)) % n]
        want = _restate_scale(w[b], v, params[b][2])
        print("M1", track, "row", b, "start", starts[b], "snr", params[b][2], "scale", float(scale[b]), "restated", want)
        assert _ulp_close(scale[b], want)
        mixed = np.clip(w[b] + v * scale[b], np.float32(-1), np.float32(1))  # float32: fl(w + fl(v * s)), then clamp
        assert mixed.dtype == np.float32 and np.array_equal(out[b], mixed)
    if track == "silent":
        assert all(float(s) == 1.0 for s in scale[:4])  # pn <= 1e-8: the host's rule
    else:
        assert float(np.abs(out[:4]).max()) == 1.0 and 0 < float(scale[3]) and float(scale[0]) < float(scale[3])
    assert float(scale[4]) == (1.0 if track == "silent" else 0.0) and np.array_equal(out[4], w[4])  # the silent clip
    print("M1", track, "row 5 left alone: max", float(np.abs(out[5]).max()))
    assert float(scale[5]) == 0.0 and np.array_equal(out[5], w[5]) and float(np.abs(out[5]).max()) == 1.5


@pytest.mark.parametrize("track", ["long", "tiled", "silent"])
def test_m2_mix_against_the_host(track):
    target = 1000
    wav, noise = _mix_rows(target), _tracks()[track]
    starts = [3, noise.numel() - 1, 200, 50, 0]
    params = [(1, starts[b], SNRS[b], 0) for b in range(4)] + [(1, starts[4], 10.0, 0), (0, 0, 0.0, 0)]
    out = clips.mix_noise_clips(wav.to(DEV), params, noise.to(DEV)).cpu().numpy()
    for b in range(5):
        host = D.mix_noise(wav[b].numpy(), noise.numpy(), starts[b], params[b][2])
        d = float(np.abs(out[b].astype(np.float64) - host.astype(np.float64)).max())
        print("M2", track, "row", b, "max |device - host|", d, "bound", 2.0 ** -22)
        assert d <= 2.0 ** -22


def test_m3_gaussian_fallback():
    n = 48000
    g = torch.Generator().manual_seed(33)
    row = torch.randn(n, generator=g) * 0.1
    wav = torch.stack([row, row, row, row])
    params = [(2, 0, 10.0, 1234567), (2, 0, 10.0, 1234567), (2, 0, 10.0, 7654321), (2, 0, 20.0, 2 ** 63 - 1)]
    out, scale = clips.mix_noise_clips(wav.to(DEV), params, return_scale=True)
    again = clips.mix_noise_clips(wav.to(DEV), params)
    assert torch.equal(out, again) and torch.equal(out[0], out[1]) and not torch.equal(out[0], out[2])
    out, scale = out.cpu().double().numpy(), scale.cpu().numpy()
    ps = float(np.mean(row.double().numpy() ** 2))
    assert float(np.abs(out).max()) < 1.0  # nothing clamped: out - wav is the noise
    for b in (0, 2, 3):
        snr = 10.0 ** (params[b][2] / 10.0)
        sigma = math.sqrt(ps / snr)
        noise = out[b] - row.double().numpy()
        mean, power = float(noise.mean()), float(np.mean(noise ** 2))
        print("M3 row", b, "sigma", float(scale[b]), "restated", sigma, "mean", mean, "bar", 4 * sigma / math.sqrt(n),
              "power / (ps / snr)", power / (ps / snr))
        assert _ulp_close(scale[b], sigma)
        assert abs(mean) <= 4 * sigma / math.sqrt(n)
        assert abs(power / (ps / snr) - 1) <= 0.03


# ------------------------------------------------------------------------------------------------ loader
def _loader_items(tmp_path):
    rng = np.random.default_rng(41)
    items, spec = [], [(48000, 2.0), (16000, 3.5), (48000, 4.0), (16000, 2.5)]  # shorter and longer than 3 s
    for i, (sr, secs) in enumerate(spec):
        frames = rng.integers(0, 256, (10 + i, 40, 48, 3), dtype=np.uint8)
        fp = tmp_path / f"f{i}.npy"
        np.save(fp, frames)
        wp = tmp_path / f"a{i}.wav"
        n = int(sr * secs)
        R.write_wav(wp, rng.normal(0, 0.3, n).clip(-1, 1) * 0.5 + 0.2 * np.sin(2 * np.pi * 440.0 * np.arange(n) / sr),
                    sr, "pcm16")
        items.append((str(fp), str(wp), i % 8, None))
    return items


def _draws(seed, n_items, n_noise):
    out = []
    for gi in range(n_items):
        rng = np.random.default_rng([seed, 0, gi])
        clips.draw_video_augment(rng)
        out.append(clips.draw_audio_augment(rng, 3 * SR, n_noise))
    return out


def test_l1_loader_plumbing(tmp_path):
    from scipy.signal import firwin, resample_poly

    items = _loader_items(tmp_path)
    bar = np.random.default_rng(42).uniform(-0.2, 0.2, 70000).astype(np.float32)  # amplitude >= 0.05
    # a seed whose draws leave a 48 kHz and a 16 kHz clip alone and augment one of each (the draws are host work)
    seed = next(s for s in range(200) if [d[0] for d in _draws(s, 4, bar.size)] in ([0, 1, 1, 0], [1, 0, 0, 1]))
    draws = _draws(seed, 4, bar.size)
    kw = dict(batch_size=4, workers=2, augment=True, bar_noise=bar, seed=seed, size=32)
    (video, audio, labels, meta), = list(D.ClipLoader(items, device_audio=True, **kw))
    (video_h, audio_h, labels_h, _), = list(D.ClipLoader(items, **kw))
    (_, mel, _, _), = list(D.ClipLoader(items, device_audio=True, audio_features="mel", **kw))
    assert tuple(audio.shape) == (4, 1, 3 * SR) and audio.is_cuda and meta["index"].tolist() == [0, 1, 2, 3]
    decoded = [D.read_wav_mono(it[1]) for it in items]
    assert [sr for _, sr in decoded] == [48000, 16000, 48000, 16000]
    hand = clips.assemble_waveforms([torch.from_numpy(w) for w, _ in decoded], [sr for _, sr in decoded], draws,
                                    torch.from_numpy(bar).to(DEV), device=DEV)
    print("L1 seed", seed, "draws", draws, "loader == by hand", torch.equal(audio, hand))
    assert torch.equal(audio, hand)
    assert torch.equal(video, video_h) and torch.equal(labels, labels_h)
    assert torch.equal(mel, clips.log_mel(audio, n_mels=64, sample_rate=SR))
    a, ah = audio[:, 0].cpu().double().numpy(), audio_h[:, 0].cpu().double().numpy()
    h = firwin(61, 1.0 / 3, window=("kaiser", 5.0))
    for b, ((w, sr), d) in enumerate(zip(decoded, draws)):
        diff = np.abs(a[b] - ah[b])
        if d[0]:
            print("L1 clip", b, sr, "augmented: max |device - host|", diff.max())
            assert diff.max() <= 1e-4
            assert np.abs(a[b] - clips.assemble_waveforms([torch.from_numpy(w)], [sr], device=DEV)[0, 0].cpu().double()
                          .numpy()).max() > 0.01  # and the noise is really there
        elif sr == SR:
            print("L1 clip", b, sr, "left alone, a copy: max |device - host|", diff.max())
            assert diff.max() == 0.0
        else:  # both sides lie within their bound of the exact result: K + 2 for the device, K + 3 for the host
            mag = np.zeros(3 * SR)
            m = resample_poly(np.abs(w.astype(np.float64)), 1, 3, window=np.abs(h))[:3 * SR]
            mag[:m.size] = m  # sum |h_k| |x_k| per output; the pad is exact on both sides
            K = 61  # up == 1: every output sums the whole filter
            bound = ((K + 2) + (K + 3)) * 2.0 ** -24 * mag
            print("L1 clip", b, sr, "left alone: max |device - host|", diff.max(), "max diff / bound",
                  float((diff / np.maximum(bound, 1e-30)).max()))
            assert bool((diff <= bound).all())


# ------------------------------------------------------------------------------------------------ timeline
@pytest.mark.parametrize("mode", ["wavlm", "xattn"])
def test_t1_timeline_takes_a_48khz_recording(mode):
    r = TL.runner(mode)
    assert r.uses_mel == (mode == "xattn")
    frames, wav = TL.recording()
    g = torch.Generator().manual_seed(51)
    wav48 = (torch.rand(TL.N_FRAMES * 48000 // TL.FPS, generator=g) - 0.5) * 0.8
    got = r.predict_timeline(frames, wav48, TL.FPS, sample_rate=48000, **TL.KW)
    wav16 = clips.resample_clips(wav48, 48000, device=DEV)
    assert tuple(wav16.shape) == (1, wav48.numel() // 3)
    want = r.predict_timeline(frames, wav16, TL.FPS, **TL.KW)
    print("T1", mode, "windows", got["num_windows"], "probs equal", torch.equal(got["probs"], want["probs"]))
    assert got["num_windows"] == want["num_windows"] > 1
    assert torch.equal(got["probs"], want["probs"]) and torch.equal(got["top1"], want["top1"])
    a, b = r.predict_timeline(frames, wav, TL.FPS, sample_rate=16000, **TL.KW), \
        r.predict_timeline(frames, wav, TL.FPS, **TL.KW)
    assert torch.equal(a["probs"], b["probs"]) and torch.equal(a["top1"], b["top1"])
    with pytest.raises(ValueError, match="positive"):
        r.predict_timeline(frames, wav, TL.FPS, sample_rate=0, **TL.KW)
    from multimodalemotionrecognition_amd.optimized_runtime import process_recording

    rows = process_recording(r, frames, wav48, TL.FPS, sample_rate=48000, **TL.KW)
    assert rows == process_recording(r, frames, wav16, TL.FPS, **TL.KW) and len(rows) == got["num_windows"]
