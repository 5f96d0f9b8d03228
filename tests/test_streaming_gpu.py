"""Live streaming sessions on the device: the three kernels of csrc/stream.hip, the session's window assembly bit for
bit, and ``StreamingSession.infer`` / ``StreamingSessionPool.infer_ready`` against the existing clip path,
``predict_probs`` on each window cut out by hand.

Bars.  Bit-exact means ``torch.equal``.  The resampler's bar against scipy's float64 ``resample_poly`` is derived, not
tuned: an output is a K-term fp32 sum of products (one fmaf per tap) whose taps were rounded to fp32 once, so it errs
by at most ``(K + 2) * 2^-24 * sum |h_k| |x_k|``.  The clip-path bar is tests/test_timeline_gpu.py's: the session and
``predict_probs`` are the same network at other batch shapes, each within 5e-3 (INT8: 1e-2) of the oracle, so within
twice that of each other."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_timeline_gpu as TL  # its recording shapes and its runners (built once per process, shared with that file)
from oracle.io_ref import uniform_indices_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
SR = 16000
CLIP_BAR, CLIP_BAR_INT8 = TL.CLIP_BAR, TL.CLIP_BAR_INT8
assert CLIP_BAR == 2 * 5e-3 and CLIP_BAR_INT8 == 2 * 1e-2
H0, W0, FPS, SECONDS, T = 36, 44, 8, 5, 4
POOL_KW = dict(window_seconds=2.0, step_seconds=0.5, max_buffer_seconds=3.0, frames_per_window=T, max_frames=16)
T0 = 100.0  # the clock's start (the reference's last_prediction_ts starts at 0.0)
_CACHE = {}


def no_launch(*a, **k):
    raise AssertionError("a launch after a bad argument")


# ------------------------------------------------------------------------------------------------ resampler
def _signal(kind, sr_in):
    if kind == "noise":
        g = torch.Generator().manual_seed(sr_in)
        return (torch.rand(4000, generator=g) - 0.5) * 0.8
    return (0.5 * torch.sin(2 * math.pi * 440.0 * torch.arange(4000, dtype=torch.float64) / sr_in)).float()


def _feed(sr_in, x, sizes, cap):
    from multimodalemotionrecognition_amd import clips

    ring = torch.zeros(cap, device=DEV)
    rs = clips.ResampleStream(sr_in, ring)
    pos, emitted = 0, 0
    for n in sizes:
        emitted += rs.push(x[pos:pos + n])
        pos += n
    assert pos == x.numel() and emitted == rs.n_out
    return rs, ring


@pytest.mark.parametrize("kind", ["noise", "tone"])
@pytest.mark.parametrize("sr_in", [48000, 44100, 8000, 16000])
def test_resample_stream(sr_in, kind):
    from scipy.signal import firwin, resample_poly

    from multimodalemotionrecognition_amd import clips

    x = _signal(kind, sr_in)
    up, down = clips.resample_ratio(sr_in, SR)
    half = 10 * max(up, down)
    assert 2 * half + 1 == {48000: 61, 44100: 8821, 8000: 41, 16000: 21}[sr_in]
    chunks = [1, 7, 300, 0, 2, 1024, 4000 - 1334]
    whole, ring_w = _feed(sr_in, x, [4000], 1000)
    parts, ring_p = _feed(sr_in, x, chunks, 1000)
    n_out = whole.n_out
    assert n_out == parts.n_out == clips.resample_emitted(4000, up, down) > 1000  # the ring wraps
    assert torch.equal(ring_w, ring_p)
    assert torch.equal(whole.counts, parts.counts) and whole.counts.tolist() == [4000, n_out]
    assert torch.equal(whole.hist, parts.hist) and whole.hist.numel() == whole.kmax
    if sr_in != SR:
        assert torch.equal(whole.hist.cpu(), x[4000 - whole.kmax:])  # the last kmax inputs
    # a ring that holds everything: the cap-1000 ring is its last 1000 outputs, output q at q % 1000
    big, ring_b = _feed(sr_in, x, chunks, 8192)
    got = ring_b[:n_out].cpu()
    q = torch.arange(n_out - 1000, n_out)
    assert torch.equal(ring_w.cpu()[q % 1000], got[q]) and float(ring_b[n_out:].abs().max()) == 0.0
    if sr_in == SR:
        assert n_out == 4000 and torch.equal(got, x)
        return
    ref = resample_poly(x.double().numpy(), up, down)
    waiting = ref.shape[0] - n_out  # outputs whose newest input has not arrived: excluded, and few
    assert 0 <= waiting <= math.ceil(half / down) + 1, waiting
    h = firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0))
    mag = resample_poly(x.double().abs().numpy(), up, down, window=np.abs(h))[:n_out]  # sum |h_k| |x_k| per output
    p = (np.arange(n_out) * down + half) % up
    K = (2 * half - p) // up + 1  # taps output o sums
    err = np.abs(got.double().numpy() - ref[:n_out])
    bound = (K + 2) * 2.0 ** -24 * mag
    print("resample", sr_in, kind, "outputs", n_out, "waiting", waiting, "max err", err.max(), "max err / bound",
          float((err / np.maximum(bound, 1e-30)).max()))
    assert bool((err <= bound).all())
    assert float(np.abs(ref[:n_out]).max()) > 0.1  # a signal, not silence


def test_resample_stream_rejects_bad_arguments(monkeypatch):
    from multimodalemotionrecognition_amd import clips
    from multimodalemotionrecognition_amd import kernels as K

    ring = torch.zeros(1000, device=DEV)
    rs = clips.ResampleStream(48000, ring)
    assert rs.push(torch.zeros(0)) == 0 and rs.n_in == 0
    monkeypatch.setattr(K, "LIB", no_launch)
    with pytest.raises(ValueError):
        rs.push(torch.zeros(10, dtype=torch.float64))
    with pytest.raises(ValueError):
        clips.ResampleStream(48000, torch.zeros(10, 10, device=DEV))
    with pytest.raises(ValueError):
        clips.ResampleStream(0, ring)
    with pytest.raises(ValueError):
        clips.ResampleStream(16000 * 64, ring)  # 256 outputs would span more inputs than a block stages
    with pytest.raises(RuntimeError):
        clips.ResampleStream(48000, torch.zeros(1000))


# ------------------------------------------------------------------------------------------------ ring windows
def test_ring_windows(monkeypatch):
    from multimodalemotionrecognition_amd import kernels as K

    g = torch.Generator().manual_seed(3)
    rings = torch.randn(3, 1000, generator=g)
    d = rings.to(DEV)
    # (slot, end, count): a short stream (padded), a window that straddles the wrap, a stream longer than its ring
    slot, end, count = [2, 0, 1], [200, 300, 500], [200, 900, 2500]
    want = torch.stack([F.pad(rings[2, :200], (0, 440)), torch.cat([rings[0, 660:], rings[0, :300]]),
                        torch.cat([rings[1, 860:], rings[1, :500]])])[:, None]
    got = K.ring_windows(d, slot, end, count, 640)
    assert got.shape == (3, 1, 640) and torch.equal(got.cpu(), want)
    got = K.ring_windows(d, torch.tensor(slot), torch.tensor(end), torch.tensor(count), 640)
    assert torch.equal(got.cpu(), want)
    # a target longer than the ring: everything held, oldest first, then zeros; end = 0: the ring is exactly full
    got = K.ring_windows(d, [1, 1], [500, 0], [2500, 1000], 1200).cpu()
    assert torch.equal(got[0, 0], F.pad(torch.cat([rings[1, 500:], rings[1, :500]]), (0, 200)))
    assert torch.equal(got[1, 0], F.pad(rings[1], (0, 200)))
    assert K.ring_windows(d, [], [], [], 640).shape == (0, 1, 640)
    monkeypatch.setattr(K, "LIB", no_launch)
    for bad in (([3], [0], [10]), ([-1], [0], [10]), ([0], [1000], [10]), ([0], [-1], [10]), ([0], [0], [-1]),
                ([0, 1], [0], [10])):
        with pytest.raises(ValueError):
            K.ring_windows(d, *bad, 640)
    with pytest.raises(ValueError):
        K.ring_windows(d, [0], [0], [10], 0)


# ------------------------------------------------------------------------------------------------ rows scatter
@pytest.mark.parametrize("D", [512, 6, 1])
def test_rows_scatter(D, monkeypatch):
    from multimodalemotionrecognition_amd import kernels as K

    g = torch.Generator().manual_seed(D)
    src = torch.randn(5, D, generator=g)
    base = torch.randn(9, D, generator=g)
    idx = torch.tensor([8, 0, 3, 7, 5], dtype=torch.int32)
    want = base.clone()
    want[idx.long()] = src
    for given in (idx, idx.tolist(), idx.long().to(DEV)):
        dst = base.to(DEV)
        assert K.rows_scatter(src.to(DEV), given, dst) is dst and torch.equal(dst.cpu(), want)
        assert torch.equal(K.rows_gather(dst, idx), src.to(DEV))  # round trip
    # 600 rows: more than one block on the vector path and on the scalar ones
    big_src = torch.randn(600, D, generator=g).to(DEV)
    perm = torch.randperm(700, generator=g)[:600]
    dst = torch.zeros(700, D, device=DEV)
    K.rows_scatter(big_src, perm, dst)
    assert torch.equal(K.rows_gather(dst, perm), big_src)
    rest = torch.ones(700, dtype=torch.bool)
    rest[perm] = False
    assert float(dst[rest.to(DEV)].abs().max()) == 0.0  # the other rows are untouched
    # views that start 4 bytes into an allocation: D % 4 == 0 but not 16-byte aligned -> the scalar path
    if D % 4 == 0:
        off_dst = torch.zeros(9 * D + 1, device=DEV)[1:].view(9, D)
        off_dst.copy_(base)
        off_src = torch.zeros(5 * D + 1, device=DEV)[1:].view(5, D)
        off_src.copy_(src)
        assert off_dst.data_ptr() % 16 == 4 and off_src.data_ptr() % 16 == 4
        assert torch.equal(K.rows_scatter(off_src, idx, off_dst).cpu(), want)
        dst = base.to(DEV)
        assert torch.equal(K.rows_scatter(off_src, idx, dst).cpu(), want)
    assert K.rows_scatter(torch.zeros(0, D, device=DEV), [], base.to(DEV)).shape == (9, D)
    monkeypatch.setattr(K, "LIB", no_launch)
    dst = base.to(DEV)
    for bad in ([8, 0, 3, 7, 8], [8, 0, 3, 7, 9], [-1, 0, 3, 7, 5], torch.tensor([0, 1, 2, 3, 3], device=DEV),
                [0, 1, 2, 3]):
        with pytest.raises(ValueError):
            K.rows_scatter(src.to(DEV), bad, dst)
    assert torch.equal(dst.cpu(), base)


# ------------------------------------------------------------------------------------------------ sessions
def recording(sr_in=SR):
    """5 s: 40 frames of 36 x 44 at 8 fps and the waveform at ``sr_in``; ``stream``: the waveform at 16 kHz as ONE
    ResampleStream push gives it (chunk-invariant by test_resample_stream), the samples every session must hold."""
    key = ("rec", sr_in)
    if key not in _CACHE:
        from multimodalemotionrecognition_amd import clips

        g = torch.Generator().manual_seed(21)
        frames = torch.randint(0, 256, (SECONDS * FPS, H0, W0, 3), generator=g, dtype=torch.uint8)
        wav = (torch.rand(SECONDS * sr_in, generator=g) - 0.5) * 0.8
        if sr_in == SR:
            stream = wav
        else:
            ring = torch.zeros(SECONDS * SR, device=DEV)
            rs = clips.ResampleStream(sr_in, ring)
            rs.push(wav)
            stream = ring[:rs.n_out].cpu()
        _CACHE[key] = (frames, wav, stream)
    return _CACHE[key]


class Restated:
    """The rules of a session restated for the test: which frames are buffered, which a window shows."""

    def __init__(self, grid, stride):
        self.grid, self.stride, self.held = grid, stride, []  # held: (ts, seq)

    def add(self, ts, seq):
        self.held.append((ts, seq))
        self.held = [f for f in self.held[-POOL_KW["max_frames"]:] if f[0] >= ts - POOL_KW["max_buffer_seconds"]]

    def pick(self, now):
        w = [q for ts, q in self.held if ts >= now - POOL_KW["window_seconds"]] or [q for _, q in self.held]
        if self.grid == "window":
            return [w[i] for i in uniform_indices_ref(len(w), T)], len(w)
        c = [q for q in w if q % self.stride == 0] or [q for _, q in self.held if q % self.stride == 0] or [self.held[-1][1]]
        c = c[-T:]
        return c + [c[-1]] * (T - len(c)), len(w)


def _events(sr_in, offset=0.0):
    """(now, sample span of a 0.1 s chunk, new frame numbers) per 0.1 s step of the recording; frame f is stamped
    T0 + offset + f / 8 and arrives in the first step at or after that."""
    n = sr_in // 10
    added = 0
    for k in range(1, SECONDS * 10 + 1):
        upto = min(SECONDS * FPS, int(math.floor(k * 0.1 * FPS + 1e-9)) + 1)  # frames with f / 8 <= k * 0.1
        yield T0 + offset + k * 0.1, ((k - 1) * n, k * n), list(range(added, upto))
        added = upto


def _window_audio(stream, n_out, target):
    n = min(n_out, target)
    return F.pad(stream[n_out - n:n_out], (0, target - n))


def _run_session(mode, grid="window", sr_in=SR, stride=None, trunk_seen=None):
    """One session over the recording in 0.1 s steps; at every tick the prediction against ``predict_probs`` on the
    window cut out by hand, and the assembly bit for bit.  Returns the pool's stats and the restated frame picks.
    ``trunk_seen``: a list that receives the batch size of every trunk call made INSIDE ``infer`` (the clip path's own
    trunk calls are not counted)."""
    from multimodalemotionrecognition_amd import clips

    r = TL.runner(mode)
    frames, wav, stream = recording(sr_in)
    pool = r.open_stream_pool(1, frame_grid=grid, frame_stride=stride, **POOL_KW)
    pool.debug = True
    ses, rule = pool.create_session(), Restated(grid, stride)
    video, audio = r.fusion_mode != "audio", r.fusion_mode != "video"
    picked, worst, ticks = [], 0.0, 0
    n_in = 0
    for now, (a, b), new in _events(sr_in):
        ses.add_audio_chunk(wav[a:b].numpy(), sr_in, timestamp=now)
        n_in = b
        for f in new:
            ses.add_frame(frames[f].numpy(), timestamp=T0 + f / FPS)
            rule.add(T0 + f / FPS, f)
        if not ses.ready_for_inference(now):
            continue
        if trunk_seen is None:
            res = ses.infer(now)
        else:  # count the frames that really reach the trunk, independently of the pool's own bookkeeping
            trunk = (r.model if r.fusion_mode == "video" else r.model.video_model).backbone
            inner = trunk.forward
            trunk.forward = lambda x: (trunk_seen.append(int(x.shape[0])), inner(x))[1]
            try:
                res = ses.infer(now)
            finally:
                del trunk.forward  # the instance attribute: the class's forward is back
        ticks += 1
        seqs, n_win = rule.pick(now)
        n_out = clips.resample_emitted(n_in, *clips.resample_ratio(sr_in, SR))
        win = _window_audio(stream, n_out, pool.target)
        clip = clips.video_clip_batch(frames[torch.tensor(seqs)][None].to(DEV))
        want = r.predict_probs(clip, win[None, None])[0]
        got = torch.tensor(res["probs"])
        worst = max(worst, float((got - want).abs().max()))
        assert res["session_id"] == ses.session_id and res["window_seconds"] == 2.0 and res["labels"] == r.labels
        assert abs(sum(res["probs"]) - 1.0) <= 1e-4 and ses.last_prediction_ts == now
        asm = pool.last_assembly
        if video:
            picked.append(seqs)
            assert res["num_buffered_frames"] == n_win
            assert asm["seqs"] == [seqs]
            held, rows = pool.debug_frames(ses.session_id)
            assert held == [q for _, q in rule.held]
            assert torch.equal(rows, clips.preprocess_frames(frames[torch.tensor(held)].to(DEV)))
            assert asm["rows"] == [q % 16 for q in seqs]
            assert torch.equal(asm["v_feat"], pool.feature_ring[torch.tensor(asm["rows"], device=DEV)][None])
        if audio:
            assert res["num_audio_samples"] == min(n_out, pool.target)
            assert torch.equal(asm["waveforms"].cpu(), win[None, None])
    assert ticks >= 6  # 2 s of audio, then every 0.5 s up to 5 s (video mode starts earlier)
    print("session", mode, grid, sr_in, "ticks", ticks, "max|dprob| against predict_probs per window", worst)
    return pool.stats, picked, worst


@pytest.mark.parametrize("mode", TL.MEL_MODES + ["wavlm", "wavlm_int8"])
def test_session_agrees_with_the_clip_path(mode):
    stats, picked, worst = _run_session(mode)
    assert worst <= (CLIP_BAR_INT8 if mode == "wavlm_int8" else CLIP_BAR)
    assert stats["predictions"] >= 6 and stats["frames_added"] == 40
    assert stats["audio_samples_resampled"] == (0 if mode == "video" else 5 * SR)  # a video checkpoint resamples nothing


def test_session_fed_48khz_chunks():
    stats, _, worst = _run_session("xattn", sr_in=48000)
    assert worst <= CLIP_BAR and stats["audio_samples_resampled"] == 5 * 48000


@pytest.mark.parametrize("grid,stride", [("window", None), ("shared", 4)])
def test_every_frame_is_encoded_once(grid, stride):
    seen = []
    stats, picked, worst = _run_session("concat", grid=grid, stride=stride, trunk_seen=seen)
    assert worst <= CLIP_BAR
    distinct = len({q for seqs in picked for q in seqs})
    assert sum(seen) == distinct and len(seen) == stats["trunk_batches"]  # what the trunk was really given
    assert stats["frames_encoded"] == distinct and stats["predictions"] == len(picked)
    assert stats["trunk_batches"] <= stats["predictions"]
    if grid == "shared":
        assert stats["frames_encoded"] < stats["predictions"] * T


def _feed_pool(pool, offsets, ticks_of=None, n_steps=None):
    """Sessions that start ``offsets`` STEPS of 0.1 s apart, fed the recording on one clock: at every step each
    running session gets its chunk and frames, then the pool is asked once.  With ``ticks_of`` None the pool decides
    (``infer_ready``, checked against the restated readiness); otherwise session ``i`` is inferred alone exactly at
    the steps ``ticks_of[i]``.  Returns the sessions and per session ``{step: probs}``."""
    frames, wav, _ = recording()
    sessions = [pool.create_session() for _ in offsets]
    events = [list(_events(SR)) for _ in offsets]
    fed = [dict(samples=0, frames=0, last=0.0) for _ in offsets]
    out = [dict() for _ in offsets]
    for step in range(1, (n_steps or SECONDS * 10 + max(offsets)) + 1):
        now = T0 + step * 0.1
        for i, off in enumerate(offsets):
            if not 1 <= step - off <= SECONDS * 10:
                continue
            _, (a, b), new = events[i][step - off - 1]
            sessions[i].add_audio_chunk(wav[a:b], SR, timestamp=now)
            for f in new:
                sessions[i].add_frame(frames[f], timestamp=T0 + off * 0.1 + f / FPS)
            fed[i]["samples"], fed[i]["frames"] = b, fed[i]["frames"] + len(new)
        if ticks_of is not None:  # (a session whose input has ended still ticks on what it holds)
            for i in range(len(offsets)):
                if step in ticks_of[i]:
                    out[i][step] = torch.tensor(sessions[i].infer(now)["probs"])
            continue
        due = {j for j, d in enumerate(fed) if d["samples"] >= 2 * SR and d["frames"] >= 2 and now - d["last"] >= 0.5}
        before = pool.stats["trunk_batches"]
        res = pool.infer_ready(now)
        assert set(res) == {sessions[j].session_id for j in due}, (step, due)
        assert pool.stats["trunk_batches"] - before <= 1
        for j in due:
            fed[j]["last"] = now
            out[j][step] = torch.tensor(res[sessions[j].session_id]["probs"])
    return sessions, out


def test_pool_predicts_the_due_sessions_in_one_batch():
    from multimodalemotionrecognition_amd import clips

    r = TL.runner("xattn")
    offsets = [0, 3, 10]  # steps of 0.1 s
    pool = r.open_stream_pool(3, **POOL_KW)
    sessions, got = _feed_pool(pool, offsets)
    assert len({s.slot for s in sessions}) == 3
    assert all(len(g) >= 6 for g in got)
    assert pool.stats["predictions"] == sum(len(g) for g in got)
    # sessions 0 and 2 start one second apart and tick every 0.5 s: due at the SAME steps, predicted in one batch
    assert len(set(got[0]) & set(got[2])) >= 4
    for i, off in enumerate(offsets):  # each row: that session inferred alone in a fresh pool, at the same instants
        solo = r.open_stream_pool(1, **POOL_KW)
        _, alone = _feed_pool(solo, [off], ticks_of=[set(got[i])], n_steps=SECONDS * 10 + max(offsets))
        assert set(alone[0]) == set(got[i])
        worst = max(float((got[i][t] - alone[0][t]).abs().max()) for t in got[i])
        print("pool session", i, "against the session alone: max|dprob|", worst)
        assert worst <= CLIP_BAR
    # a closed session's slot is reused, and the new session sees none of the old state
    old = sessions[0]
    pool.close_session(old.session_id)
    assert old.session_id not in pool.sessions
    frames, wav, _ = recording()
    for late in (lambda: old.add_frame(frames[0], timestamp=T0 + 50.0), lambda: old.add_audio_chunk(wav[:160], SR),
                 lambda: old.infer(T0 + 50.0)):
        with pytest.raises(RuntimeError, match="closed"):  # a handler racing the disconnect gets a clear error
            late()
    new = pool.create_session()
    assert new.slot == old.slot and not new.ready_for_inference(T0 + 50.0)
    frames, wav, _ = recording()
    new.add_frame(frames[5], timestamp=T0 + 50.0)
    new.add_frame(frames[6], timestamp=T0 + 50.1)
    new.add_audio_chunk(wav[:3000], SR)
    pool.debug = True
    res = new.infer(T0 + 50.2)
    assert res["num_buffered_frames"] == 2 and res["num_audio_samples"] == 3000
    asm = pool.last_assembly
    assert asm["seqs"] == [[0, 1, 1, 1]]
    assert torch.equal(asm["waveforms"].cpu()[0, 0], F.pad(wav[:3000], (0, pool.target - 3000)))
    held, rows = pool.debug_frames(new.session_id)
    assert held == [0, 1] and torch.equal(rows, clips.preprocess_frames(frames[5:7].to(DEV)))
    fresh = r.open_stream_pool(1, **POOL_KW)
    f = fresh.create_session()
    f.add_frame(frames[5], timestamp=T0 + 50.0)
    f.add_frame(frames[6], timestamp=T0 + 50.1)
    f.add_audio_chunk(wav[:3000], SR)
    want = f.infer(T0 + 50.2)
    assert float((torch.tensor(res["probs"]) - torch.tensor(want["probs"])).abs().max()) <= CLIP_BAR
    with pytest.raises(RuntimeError):
        [pool.create_session() for _ in range(2)]  # three slots, three in use after the first
