"""Face-box crops, the host half (no device): ``clips.crop_rects`` against ``data.face_crop_box`` and against a
restatement of the reference's ``crop_with_padding`` (face_crop.py:151-190) written out here, the descriptor table of
``clips.crop_resize_frames``, and every argument refusal of the new surface, each raised before any device work."""
import numpy as np
import pytest
import torch

H, W = 90, 160


def crop_with_padding_ref(frame, bbox, pad_ratio=0.3):
    """face_crop.py's crop_with_padding, restated: pad each side by int(side * pad_ratio), clip to the frame, slice."""
    h, w = frame.shape[:2]
    x1, y1, x2, y2 = bbox
    bw, bh = x2 - x1, y2 - y1
    pad_x, pad_y = int(bw * pad_ratio), int(bh * pad_ratio)
    x1p, y1p = max(0, x1 - pad_x), max(0, y1 - pad_y)
    x2p, y2p = min(w, x2 + pad_x), min(h, y2 + pad_y)
    return frame[y1p:y2p, x1p:x2p]


BOXES = {
    "inside": (60, 30, 100, 70),
    "past_left": (-20, 30, 40, 70),
    "past_top": (60, -15, 100, 30),
    "past_right": (120, 30, 175, 70),
    "past_bottom": (60, 50, 100, 110),
    "whole_frame": (10, 5, 150, 85),  # pad 42 x 24 reaches past every edge
    "odd": (7, 3, 20, 12),
}


def test_crop_rects_is_face_crop_box_row_by_row():
    from multimodalemotionrecognition_amd import clips
    from multimodalemotionrecognition_amd.data import face_crop_box

    names = list(BOXES)
    for pad in (0.3, 0.0, 0.5):
        got = clips.crop_rects(H, W, [BOXES[k] for k in names], pad)
        assert got.dtype == np.int64 and got.shape == (len(names), 4)
        for k, row in zip(names, got):
            assert tuple(row) == face_crop_box(H, W, BOXES[k], pad), (k, pad)
    as_array = clips.crop_rects(H, W, np.array([BOXES[k] for k in names], dtype=np.int32))
    as_tensor = clips.crop_rects(H, W, torch.tensor([BOXES[k] for k in names]))
    assert np.array_equal(as_array, clips.crop_rects(H, W, [BOXES[k] for k in names]))
    assert np.array_equal(as_tensor, as_array)
    assert clips.crop_rects(H, W, []).shape == (0, 4)


def test_crop_rects_pinned_cases():
    from multimodalemotionrecognition_amd import clips

    rect = lambda b, pad=0.3: tuple(int(v) for v in clips.crop_rects(H, W, [b], pad)[0])
    assert rect(BOXES["inside"]) == (48, 18, 112, 82)  # pad int(40 * 0.3) = 12 on every side
    assert rect(BOXES["past_left"]) == (0, 18, 58, 82)  # pad 18 x 12
    assert rect(BOXES["past_top"]) == (48, 0, 112, 43)  # pad 12 x 13
    assert rect(BOXES["past_right"]) == (104, 18, 160, 82)  # pad 16 x 12
    assert rect(BOXES["past_bottom"]) == (48, 32, 112, 90)  # pad 12 x 18
    assert rect(BOXES["whole_frame"]) == (0, 0, W, H)  # the padded rectangle IS the whole frame
    # an empty box (no detection), an inverted one, and None: the whole frame, select_frames's rule
    assert rect((0, 0, 0, 0)) == (0, 0, W, H)
    assert rect((50, 40, 50, 60)) == (0, 0, W, H)
    assert rect((80, 40, 60, 60)) == (0, 0, W, H)
    assert rect((300, 200, 340, 240)) == (0, 0, W, H)  # a box outside the frame clips to nothing
    assert rect(None) == (0, 0, W, H)
    mixed = clips.crop_rects(H, W, [None, BOXES["inside"], (0, 0, 0, 0)])
    assert mixed.tolist() == [[0, 0, W, H], [48, 18, 112, 82], [0, 0, W, H]]


@pytest.mark.parametrize("name", list(BOXES))
def test_rect_has_the_shape_of_crop_with_padding(name):
    from multimodalemotionrecognition_amd import clips
    from multimodalemotionrecognition_amd.data import select_frames

    frame = np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)
    for pad in (0.3, 0.1):
        x1, y1, x2, y2 = clips.crop_rects(H, W, [BOXES[name]], pad)[0]
        want = crop_with_padding_ref(frame, BOXES[name], pad)
        assert want.size and frame[y1:y2, x1:x2].shape == want.shape and np.array_equal(frame[y1:y2, x1:x2], want)
        # and it is what the loader's host path cuts out
        assert np.array_equal(select_frames(frame[None], 1, BOXES[name], pad)[0], want)


def test_crop_rects_refusals():
    from multimodalemotionrecognition_amd import clips

    for bad in ([(1.5, 2, 30, 40)], [(1, 2, 3)], [(1, 2, 3, 4, 5)], ["abcd"], [7], np.zeros((2, 3), dtype=np.int64),
                np.zeros((2, 4), dtype=np.float32), [(0, 0, 2 ** 31, 5)]):
        with pytest.raises(ValueError):
            clips.crop_rects(H, W, bad)
    with pytest.raises(ValueError):
        clips.crop_rects(0, W, [None])


def test_crop_rows_layout():
    from multimodalemotionrecognition_amd import clips

    rows = clips.crop_rows([0, 105, 105], [5, 33, 33], [7, 129, 129],
                           [[0, 0, 7, 5], [1, 2, 100, 30], [128, 32, 129, 33]])
    assert rows.dtype == np.int64 and rows.tolist() == [[0, 5, 7, 0, 0, 7, 5, 0], [105, 33, 129, 1, 2, 100, 30, 0],
                                                        [105, 33, 129, 128, 32, 129, 33, 0]]
    one_size = clips.crop_rows(torch.tensor([0, 300]), 10, 10, [[0, 0, 10, 10], [2, 2, 4, 4]])
    assert one_size[:, 1:3].tolist() == [[10, 10], [10, 10]] and one_size[:, 0].tolist() == [0, 300]
    with pytest.raises(ValueError):
        clips.crop_rows([0], 10, 10, [[0, 0, 10, 10], [2, 2, 4, 4]])


def _no_device(monkeypatch):
    """Any launch or upload after a bad argument fails the test."""
    from multimodalemotionrecognition_amd import clips
    from multimodalemotionrecognition_amd import kernels as K

    def boom(*a, **k):
        raise AssertionError("device work after a bad argument")

    monkeypatch.setattr(K, "LIB", boom)
    monkeypatch.setattr(clips, "_h2d", boom)


def test_crop_resize_frames_validates_rows_on_the_host(monkeypatch):
    from multimodalemotionrecognition_amd import clips

    _no_device(monkeypatch)
    buf = torch.zeros(5 * 7 * 3 + 10, dtype=torch.uint8)  # a host buffer: a valid table reaches the device check
    ok = [0, 5, 7, 0, 0, 7, 5, 0]
    bad_rows = [
        [-1, 5, 7, 0, 0, 7, 5, 0],  # offset before the buffer
        [11, 5, 7, 0, 0, 7, 5, 0],  # image ends past the buffer
        [0, 6, 7, 0, 0, 7, 5, 0],  # image larger than the buffer
        [0, 0, 7, 0, 0, 7, 5, 0], [0, 5, 0, 0, 0, 7, 5, 0],  # empty image
        [0, 5, 7, 0, 0, 8, 5, 0], [0, 5, 7, 0, 0, 7, 6, 0],  # rectangle past the right / bottom edge
        [0, 5, 7, -1, 0, 7, 5, 0], [0, 5, 7, 0, -1, 7, 5, 0],  # negative origin
        [0, 5, 7, 3, 0, 3, 5, 0], [0, 5, 7, 0, 4, 7, 4, 0], [0, 5, 7, 5, 0, 4, 5, 0],  # empty / inverted rectangle
        [0, 5, 7, 0, 0, 7, 5, 1],  # the reserved column
        [0, 1 << 25, 1, 0, 0, 1, 1, 0],  # a side beyond what the kernel's int offsets hold
    ]
    for row in bad_rows:
        with pytest.raises(ValueError):
            clips.crop_resize_frames(buf, [ok, row])
    for rows in ([[0, 5, 7, 0, 0, 7]], np.zeros((1, 8), dtype=np.float32), [0, 5, 7, 0, 0, 7, 5, 0]):
        with pytest.raises(ValueError):
            clips.crop_resize_frames(buf, rows)
    for size in (0, -3, 16 * 65535 + 1):
        with pytest.raises(ValueError):
            clips.crop_resize_frames(buf, [ok], size=size)
    with pytest.raises(ValueError):
        clips.crop_resize_frames(buf.view(5, -1), [ok])
    with pytest.raises(ValueError):
        clips.crop_resize_frames(buf.float(), [ok])
    with pytest.raises(RuntimeError):  # everything valid: only now is the device asked for
        clips.crop_resize_frames(buf, [ok])
    with pytest.raises(RuntimeError):
        clips.crop_resize_frames(buf, [ok[:7]])  # the seven-column form


def test_pack_frames_and_gather_refusals(monkeypatch):
    from multimodalemotionrecognition_amd import clips

    _no_device(monkeypatch)
    a = np.zeros((2, 4, 5, 3), dtype=np.uint8)
    for bad in ([a.astype(np.float32)], [a[0]], [a[..., :2]], ["x"]):
        with pytest.raises(ValueError):
            clips.pack_frames(bad, device="cuda")
    with pytest.raises(ValueError):
        clips.pack_frames([], device="cuda")
    with pytest.raises(RuntimeError):
        clips.pack_frames([a], device="cpu")
    with pytest.raises(RuntimeError):
        clips.gather_preprocess_frames(torch.from_numpy(a), [0], 16, rects=[[0, 0, 5, 4]])


def test_library_rejects_bad_arguments_without_a_launch():
    """mer_frames_crop_resize returns hipErrorInvalidValue (1) before any HIP call, so this runs without a GPU."""
    from multimodalemotionrecognition_amd._lib import LIB

    LIB.load()
    f = LIB._fns["mer_frames_crop_resize"]
    fake = 1 << 20  # never dereferenced
    norm = (0.485, 0.456, 0.406, 0.229, 0.224, 0.225)
    assert f(None, 100, 1, fake, 112, 0, *norm, fake, None) == 1
    assert f(fake, 100, 1, None, 112, 0, *norm, fake, None) == 1
    assert f(fake, 100, 1, fake, 112, 0, *norm, None, None) == 1
    assert f(fake, 100, 1, fake, 0, 0, *norm, fake, None) == 1
    assert f(fake, 100, -1, fake, 112, 0, *norm, fake, None) == 1
    assert f(fake, 100, 1, fake, 112, 2, *norm, fake, None) == 1
    assert f(fake, 2, 1, fake, 112, 0, *norm, fake, None) == 1
    assert f(fake, 100, 0, fake, 112, 0, *norm, fake, None) == 0  # nothing to do: no launch
    assert f(fake, 100, 0, fake, 112, 1, *norm, fake, None) == 0


def test_face_boxes_argument():
    from multimodalemotionrecognition_amd.timeline import checked_face_boxes

    assert checked_face_boxes(None, 10) is None
    assert checked_face_boxes((1, 2, 3, 4), 10).tolist() == [[1, 2, 3, 4]]
    assert checked_face_boxes(torch.tensor([1, 2, 3, 4], dtype=torch.int32), 10).tolist() == [[1, 2, 3, 4]]
    table = np.arange(40, dtype=np.int32).reshape(10, 4)
    got = checked_face_boxes(table, 10)
    assert got.dtype == np.int64 and np.array_equal(got, table)
    for bad in ((1.0, 2, 3, 4), np.zeros((9, 4), dtype=np.int64), np.zeros((10, 4), dtype=np.float32), [1, 2, 3],
                np.zeros((10, 5), dtype=np.int64), "box", np.zeros((1, 10, 4), dtype=np.int64),
                torch.zeros(10, 4), (0, 0, 2 ** 31, 4)):
        with pytest.raises(ValueError):
            checked_face_boxes(bad, 10)


def _cpu_runner(mode):
    from multimodalemotionrecognition_amd.optimized_runtime import TorchModelRunner
    from multimodalemotionrecognition_amd.train import build_model

    torch.manual_seed(0)
    src = build_model(8, mode, pretrained_video=False, use_wavlm=False, use_resnet_audio=False)
    return TorchModelRunner(checkpoint={"model": src.state_dict()}, device="cpu")


def test_predict_timeline_refuses_bad_boxes_before_any_device_work():
    """On a CPU runner the device refusal (RuntimeError) comes after the argument checks: a bad ``face_boxes`` must
    raise ValueError first, and a good one must get as far as the device refusal."""
    from multimodalemotionrecognition_amd.optimized_runtime import process_recording

    frames = torch.zeros(12, 20, 24, 3, dtype=torch.uint8)
    wav = torch.zeros(24000)
    video, audio = _cpu_runner("video"), _cpu_runner("audio")
    for bad in ((1.0, 2.0, 3.0, 4.0), np.zeros((11, 4), dtype=np.int64), np.zeros((12, 4), dtype=np.float64),
                [[1, 2, 3, 4]] * 3, "box"):
        with pytest.raises(ValueError):
            video.predict_timeline(frames, wav, 8, face_boxes=bad)
        with pytest.raises(ValueError):
            process_recording(video, frames, wav, 8, face_boxes=bad)
    with pytest.raises(ValueError, match="audio-only"):
        audio.predict_timeline(frames, wav, 8, face_boxes=(1, 2, 10, 12))
    with pytest.raises(ValueError, match="audio-only"):
        audio.predict_timeline(None, wav, 8, face_boxes=(1, 2, 10, 12))
    with pytest.raises(RuntimeError):
        video.predict_timeline(frames, wav, 8, face_boxes=(1, 2, 10, 12))
    with pytest.raises(RuntimeError):
        video.predict_timeline(frames, wav, 8, face_boxes=np.zeros((12, 4), dtype=np.int32), pad_ratio=0.2)


def test_streaming_bbox_is_checked_before_the_frame_is_stored():
    from multimodalemotionrecognition_amd.streaming import StreamingSession, StreamState

    class Pool:  # the device half must not be reached
        pad_ratio = 0.3

        def _store_frame(self, *a):
            raise AssertionError("stored a frame after a bad box")

    s = StreamingSession(Pool(), 0, StreamState())
    frame = np.zeros((20, 24, 3), dtype=np.uint8)
    for bad in ((1.5, 2, 3, 4), (1, 2, 3), "abcd", 7):
        with pytest.raises(ValueError):
            s.add_frame(frame, 1.0, bbox=bad)
    assert s.state.next_seq == 0 and not s.state.frames


def test_loader_device_video_needs_a_gpu_device():
    from multimodalemotionrecognition_amd.data import ClipLoader

    assert ClipLoader([], device="cpu").device_video is False
    with pytest.raises(RuntimeError):
        ClipLoader([], device="cpu", device_video=True)
