"""Host control plane of the live streaming sessions (streaming.StreamState / StreamingSession) against a restatement
of the reference session, the frame choice of both grids, the resampler's polyphase table and emitted-count closed
form, and the argument errors that must come before any device work.  No device."""
import math
from collections import deque

import numpy as np
import pytest
import torch

from multimodalemotionrecognition_amd import clips
from multimodalemotionrecognition_amd import streaming as S
from oracle.io_ref import uniform_indices_ref

SR = 16000


class RefSession:
    """backend/app/streaming.py:55-117 restated: host deques, whole-chunk audio pruning, the three readiness terms."""

    def __init__(self, window, step, max_buffer):
        self.window, self.step, self.max_buffer = window, step, max_buffer
        self.frames, self.chunks, self.count, self.last, self.sr = deque(), deque(), 0, 0.0, SR

    def add_frame(self, ts):
        self.frames.append(ts)
        while self.frames and self.frames[0] < ts - self.max_buffer:
            self.frames.popleft()

    def add_audio(self, n, sr):
        self.sr = sr
        self.chunks.append(n)
        self.count += n
        while self.count > max(1, int(self.sr * self.max_buffer)) and self.chunks:
            self.count -= self.chunks.popleft()

    def ready(self, now):
        return self.count >= int(self.sr * self.window) and len(self.frames) >= 2 and (now - self.last) >= self.step

    def window_frames(self, now):
        return [t for t in self.frames if t >= now - self.window] or list(self.frames)

    def infer(self, now):
        self.last = now
        return dict(num_buffered_frames=len(self.window_frames(now)), num_audio_samples=min(self.count, int(self.sr * self.window)))


class FakePool:
    """The pool's three hooks on the host state alone: what a session calls, without the device half."""

    def __init__(self):
        self.calls = []

    def _store_frame(self, s, frame, now):
        s.state.add_frame(now)

    def _store_audio(self, s, flat, sr):
        s.state.add_audio(int(flat.numel()), sr)

    def _infer(self, sessions, now):
        out = {}
        for s in sessions:
            seqs, n_win = s.state.select(now)
            s.state.last_prediction_ts = now
            self.calls.append((now, seqs))
            out[s.session_id] = dict(num_buffered_frames=n_win, num_audio_samples=min(s.state.audio_window()[1], s.state.target))
        return out


def test_cadence_and_pruning_follow_the_reference():
    kw = dict(window_seconds=2.0, step_seconds=0.5, max_buffer_seconds=3.0)
    ref = RefSession(2.0, 0.5, 3.0)
    ses = S.StreamingSession(FakePool(), 0, S.StreamState(frames_per_window=4, max_frames=64, **kw))
    frame = np.zeros((4, 5, 3), dtype=np.uint8)
    chunk = np.zeros(800, dtype=np.float32)  # 50 ms at 16 kHz
    n_ready = n_pred = 0
    for k in range(1, 241):  # 12 s in 50 ms events, from t = 100 (the reference's last_prediction_ts starts at 0)
        now = 100.0 + k * 0.05
        if not 5.0 <= k * 0.05 < 7.5:  # the audio stops for 2.5 s
            ref.add_audio(800, SR)
            ses.add_audio_chunk(chunk, SR, timestamp=now)
        if k % 3 == 0 and not 3.0 <= k * 0.05 < 4.0 and k * 0.05 < 9.0:  # ~6.7 fps with a 1 s gap, none after 9 s
            ref.add_frame(now)
            ses.add_frame(frame, timestamp=now)
        assert [t for t, _ in ses.state.frames] == list(ref.frames), k
        r = ref.ready(now)
        assert ses.ready_for_inference(now) == r, (k, now)
        n_ready += r
        if r and k % 3 == 0:  # the caller polls every 150 ms: some ready instants pass unpolled
            want, got = ref.infer(now), ses.infer(now)
            assert got == want and ses.last_prediction_ts == ref.last == now
            n_pred += 1
    # first prediction once 2 s of audio are in; then every 0.5 s: the script must exercise both answers
    assert n_pred >= 15 and n_ready > n_pred
    # frames stopped at 9 s: the buffer keeps what the last add_frame left (pruning happens on arrival, as there)
    assert len(ses.state.frames) == len(ref.frames) >= 2
    # not ready: too little audio, one frame, step not elapsed
    st = S.StreamState(frames_per_window=4, max_frames=8, **kw)
    st.add_frame(1.0), st.add_frame(1.1)
    st.add_audio(2 * SR - 1, SR)
    assert not st.ready(10.0)
    st.add_audio(1, SR)
    assert st.ready(10.0)
    st.last_prediction_ts = 9.6
    assert not st.ready(10.0) and st.ready(10.1)
    one = S.StreamState(frames_per_window=4, max_frames=8, **kw)
    one.add_frame(1.0), one.add_audio(3 * SR, SR)
    assert not one.ready(10.0)
    # a single-modality runner waits for its own modality only
    a = S.StreamState(frames_per_window=4, max_frames=8, need_frames=False, **kw)
    a.add_audio(2 * SR, SR)
    assert a.ready(10.0)


def _ref_window(frames, now, window):
    w = [q for ts, q in frames if ts >= now - window] or [q for _, q in frames]
    return w


@pytest.mark.parametrize("case", ["inside", "none_inside", "fewer_than_T", "overwrite"])
def test_window_grid_is_uniform_indices_over_the_window(case):
    T = 4
    st = S.StreamState(window_seconds=2.0, step_seconds=0.5, max_buffer_seconds=3.0, frames_per_window=T, max_frames=16)
    if case == "inside":
        stamps, now = [k / 8 for k in range(24)], 3.0  # 3 s at 8 fps: window [1.0, 3.0] holds seq 8..23
    elif case == "none_inside":
        stamps, now = [k / 8 for k in range(6)], 5.0  # all frames older than now - 2 s: every buffered frame
    elif case == "fewer_than_T":
        stamps, now = [0.0, 0.1, 2.5, 2.9], 3.0  # two frames in the window
    else:
        stamps, now = [k / 20 for k in range(50)], 2.5  # 20 fps: 40 frames in the window, the ring keeps 16
    held = deque()
    for q, ts in enumerate(stamps):
        slot = st.add_frame(ts)
        assert slot == q % 16
        held.append((ts, q))
        while len(held) > 16 or held[0][0] < ts - 3.0:
            held.popleft()
    assert list(st.frames) == list(held)
    assert len({st.slot_of(q) for _, q in st.frames}) == len(st.frames)  # no two buffered frames share a slot
    w = _ref_window(held, now, 2.0)
    seqs, n_win = st.select(now)
    assert n_win == len(w) and seqs == [w[i] for i in uniform_indices_ref(len(w), T)]
    assert len(seqs) == T
    if case == "overwrite":
        assert [q for _, q in st.frames] == list(range(34, 50)) and min(seqs) == 34 and max(seqs) == 49
    if case == "fewer_than_T":
        assert seqs == [2, 3, 3, 3]
    if case == "none_inside":
        assert seqs == [0, 2, 3, 5]


def test_shared_grid_consecutive_ticks_share_frames():
    st = S.StreamState(window_seconds=2.0, step_seconds=0.5, max_buffer_seconds=3.0, frames_per_window=4,
                       max_frames=32, frame_grid="shared", frame_stride=4)
    for q in range(28):  # 8 fps: frame q at q / 8 s
        st.add_frame(q / 8)
    a, _ = st.select(3.0)  # frames at or after 1.0 s: seq 8..27, eligible 8, 12, ..., 24: the last 4
    for q in range(28, 32):
        st.add_frame(q / 8)
    b, _ = st.select(3.5)
    assert a == [12, 16, 20, 24] and b == [16, 20, 24, 28] and len(set(a) & set(b)) == 3
    # fewer eligible frames than T: each once, the last repeated; none eligible in the window: the buffered ones
    few = S.StreamState(window_seconds=2.0, max_buffer_seconds=3.0, frames_per_window=4, max_frames=32,
                        frame_grid="shared", frame_stride=4)
    for q in range(6):
        few.add_frame(q / 8)
    assert few.select(0.7)[0] == [0, 4, 4, 4]
    assert few.select(2.55)[0] == [0, 4, 4, 4]  # the window [0.55, 2.55] holds seq 5 only, no multiple of 4
    assert few.select(9.0)[0] == [0, 4, 4, 4]  # nothing inside: every buffered frame
    with pytest.raises(ValueError):
        S.StreamState(frame_grid="shared")
    with pytest.raises(ValueError):
        S.StreamState(frame_grid="clip")


@pytest.mark.parametrize("sr_in", [48000, 44100, 8000, 22050])
def test_polyphase_table_is_the_kaiser_firwin_by_phase(sr_in):
    from scipy.signal import firwin

    up, down = clips.resample_ratio(sr_in, SR)
    assert (up, down) == {48000: (1, 3), 44100: (160, 441), 8000: (2, 1), 22050: (320, 441)}[sr_in]
    half = 10 * max(up, down)
    g = (firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up).astype(np.float32)
    tab = clips.polyphase_table(up, down)
    kmax = 2 * half // up + 1
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (up, kmax)
    want = np.zeros((up, kmax), dtype=np.float32)
    for k in range(2 * half + 1):
        want[k % up, k // up] = g[k]
    assert np.array_equal(tab.numpy(), want)
    assert abs(float(tab.double().sum()) - up) < 1e-4 * up  # unit DC gain times up


@pytest.mark.parametrize("sr_in", [48000, 44100, 8000, 22050, 16000])
def test_emitted_count_is_the_closed_form(sr_in):
    up, down = clips.resample_ratio(sr_in, SR)
    half = 10 * max(up, down)

    def brute(n):  # outputs whose newest input floor((o * down + half) / up) is below n
        if up == down == 1:
            return n
        o = 0
        while (o * down + half) // up <= n - 1:
            o += 1
        return o

    for n in (0, 1, 2, 29, 30, 31, 61, 100, 441, 1000, 4000):
        e = clips.resample_emitted(n, up, down)
        assert e == brute(n), n
        # never ahead of resample_poly's ceil(n * up / down) outputs, behind by the filter's half length at most
        assert 0 <= -(-n * up // down) - e <= (0 if up == down == 1 else math.ceil(half / down) + 1)
    for sizes in ([4000], [1, 7, 300, 0, 2, 1024, 2666], [1] * 50 + [0, 0, 3950], [0, 4000, 0]):
        st = S.StreamState()
        got = [st.add_audio(n, sr_in) for n in sizes]
        assert sum(sizes) == 4000 == st.n_in
        assert sum(got) == st.n_out == clips.resample_emitted(4000, up, down)
        assert all(v >= 0 for v in got)


def test_argument_errors_come_before_device_work():
    from multimodalemotionrecognition_amd import optimized_runtime as R
    from multimodalemotionrecognition_amd.train import build_model

    src = build_model(8, "audio", use_wavlm=False, use_resnet_audio=False)
    runner = R.TorchModelRunner(checkpoint={"model": src.state_dict()}, device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        runner.open_stream_pool(4)
    with pytest.raises(RuntimeError, match="GPU"):
        S.StreamingSessionPool(runner, 4)
    with pytest.raises(ValueError, match="max_frames"):
        S.StreamState(frames_per_window=8, max_frames=7)
    with pytest.raises(ValueError):
        S.StreamState(window_seconds=3.0, max_buffer_seconds=2.0)

    class NoDevice:  # any device work would be an AttributeError, not the ValueError asked for
        pass

    ses = S.StreamingSession(NoDevice(), 0, S.StreamState())
    for bad in (np.zeros((4, 4, 3), dtype=np.float32), torch.zeros(4, 4, 3), np.zeros((4, 4), dtype=np.uint8),
                np.zeros((4, 4, 4), dtype=np.uint8), "frame"):
        with pytest.raises(ValueError):
            ses.add_frame(bad, timestamp=1.0)
    assert not ses.state.frames
    ses.state.add_audio(480, 48000)  # the first chunk fixed the rate
    with pytest.raises(ValueError, match="48000"):
        ses.add_audio_chunk(np.zeros(160, dtype=np.float32), 16000)
    with pytest.raises(ValueError):
        ses.add_audio_chunk(np.zeros(160, dtype=np.float32), 0)
    assert ses.state.n_in == 480
    # integer PCM is refused (the reference scales it to [-1, 1] first), and so is anything that is not an array
    for bad in (np.zeros(160, dtype=np.int16), torch.zeros(160, dtype=torch.int32), "chunk"):
        with pytest.raises(ValueError):
            ses.add_audio_chunk(bad, 48000)
    assert ses.state.n_in == 480
    # a closed session says so
    closed = S.StreamingSession(None, 0, S.StreamState())
    for late in (lambda: closed.add_frame(np.zeros((4, 4, 3), dtype=np.uint8), timestamp=1.0),
                 lambda: closed.add_audio_chunk(np.zeros(160, dtype=np.float32), 16000), lambda: closed.infer(1.0)):
        with pytest.raises(RuntimeError, match="closed"):
            late()


def test_entry_points_reject_bad_arguments_before_any_launch():
    """hipErrorInvalidValue (1) or 0 for empty work, before any HIP call: runs without a GPU."""
    from multimodalemotionrecognition_amd._lib import LIB

    LIB.load()
    f = LIB._fns
    fake = 1 << 20  # never dereferenced
    # mer_resample_stream(up, down, kmax, table, chunk, n_chunk, n_in, hist, hist_new, hist_len, ring, cap, counts, st)
    ok = [1, 3, 61, fake, fake, 100, 0, fake, fake + 4096, 61, fake, 1000, fake, None]
    assert f["mer_resample_stream"](*(ok[:5] + [0] + ok[6:])) == 0  # an empty chunk: nothing to do
    for pos, bad in ((0, 0), (1, -3), (2, 60), (3, None), (4, None), (5, -1), (6, -1), (7, None), (8, fake), (9, 60),
                     (10, None), (11, 0), (12, None)):
        args = list(ok)
        args[pos] = bad
        assert f["mer_resample_stream"](*args) == 1, pos
    assert f["mer_resample_stream"](1, 200, 4001, fake, fake, 100, 0, fake, fake + 65536, 4001, fake, 1000, fake,
                                    None) == 1  # 256 outputs would span more inputs than a block stages
    # mer_ring_windows(B, target, rings, n_slots, cap, slot, end, count, out, stream)
    assert f["mer_ring_windows"](0, 640, fake, 3, 1000, fake, fake, fake, fake, None) == 0
    assert f["mer_ring_windows"](3, 640, fake, 3, 1000, None, fake, fake, fake, None) == 1
    assert f["mer_ring_windows"](3, 640, fake, 0, 1000, fake, fake, fake, fake, None) == 1
    assert f["mer_ring_windows"](65536, 640, fake, 3, 1000, fake, fake, fake, fake, None) == 1
    # mer_rows_scatter(n_dst, n_rows, D, src, idx, dst, stream)
    assert f["mer_rows_scatter"](5, 0, 512, fake, fake, fake, None) == 0
    assert f["mer_rows_scatter"](5, 4, 512, fake, None, fake, None) == 1
    assert f["mer_rows_scatter"](0, 4, 512, fake, fake, fake, None) == 1
