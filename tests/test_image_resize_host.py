"""Host half of the device resize (emote_hack_amd.video_io.resize_taps, resize_frames' refusals, load_control_clip's frame arithmetic):
the tables are right when a plain numpy restatement on them (tests/image_resize_ref.py) gives Pillow's bytes.  Every comparison is an
equality.  No device is needed."""
import numpy as np
import pytest
import torch

from emote_hack_amd import video_io as V
from tests import image_resize_ref as R


@pytest.mark.parametrize("name", R.FILTERS)
@pytest.mark.parametrize("shape_in,shape_out", R.SHAPES)
def test_restatement_on_the_tables_equals_pillow(name, shape_in, shape_out):
    frame = R.make_frames("noise", 1, *shape_in)[0]
    assert np.array_equal(R.resize(frame, *shape_out, name), R.pillow_resize(frame, *shape_out, name))


def test_hamming_constants_are_single_precision():
    # the rows where the double constants 0.54 / 0.46 would round a coefficient the other way (1080 -> 512)
    frame = R.make_frames("noise", 1, 1080, 64)[0]
    assert np.array_equal(R.resize(frame, 512, 64, "hamming"), R.pillow_resize(frame, 512, 64, "hamming"))


def test_pillow_without_a_filter_is_bicubic():
    for shape_in, shape_out in R.SHAPES:
        frame = R.make_frames("noise", 1, *shape_in)[0]
        assert np.array_equal(R.pillow_resize(frame, *shape_out), R.resize(frame, *shape_out, "bicubic"))
    assert V.resize_taps(37, 64)[1] is V.resize_taps(37, 64, "bicubic")[1]


@pytest.mark.parametrize("name,support", [("box", 0.5), ("bilinear", 1.0), ("hamming", 1.0), ("bicubic", 2.0), ("lanczos", 3.0)])
def test_table_shapes_dtypes_and_cache(name, support):
    for in_size, out_size in ((53, 64), (64, 24), (300, 5), (1, 16), (16, 16)):
        bounds, coef = V.resize_taps(in_size, out_size, name)
        ksize = int(np.ceil(support * max(in_size / out_size, 1.0))) * 2 + 1
        assert bounds.dtype == np.int32 and bounds.shape == (out_size, 2)
        assert coef.dtype == np.int32 and coef.shape == (out_size, ksize)
        assert not bounds.flags.writeable and not coef.flags.writeable
        first, count = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
        assert (first >= 0).all() and (count >= 1).all() and (count <= ksize).all() and (first + count <= in_size).all()
        assert all((coef[o, count[o]:] == 0).all() for o in range(out_size))                  # zero behind the taps
        assert (np.abs(coef.astype(np.int64).sum(axis=1) - (1 << 22)) <= ksize).all()         # weights sum to 1, each rounded once
        again = V.resize_taps(in_size, out_size, name.upper())
        assert again[0] is bounds and again[1] is coef                                        # cached, whatever the letter case
    assert V.RESIZE_FILTERS[name][1] == support


def test_refusals():
    frame = np.zeros((8, 8, 3), np.uint8)
    for bad in ("nearest", "NEAREST"):
        with pytest.raises(ValueError, match="nearest-neighbour resizing is not built"):
            V.resize_taps(8, 4, bad)
        with pytest.raises(ValueError, match="nearest-neighbour resizing is not built"):
            V.resize_frames(frame, (4, 4), resample=bad)
    with pytest.raises(ValueError, match="resample= takes one of"):
        V.resize_taps(8, 4, "gaussian")
    with pytest.raises(ValueError, match="resample= takes one of"):
        V.resize_taps(8, 4, 3)
    with pytest.raises(ValueError, match="box= .* not built"):
        V.resize_frames(frame, (4, 4), box=(0, 0, 4, 4))
    with pytest.raises(ValueError, match="reducing_gap= .* not built"):
        V.resize_frames(frame, (4, 4), reducing_gap=2.0)
    with pytest.raises(ValueError, match="positive ints"):
        V.resize_taps(0, 4)
    with pytest.raises(ValueError, match=r"size=\(width, height\)"):
        V.resize_frames(frame, (4, 0))
    with pytest.raises(ValueError, match=r"size=\(width, height\)"):
        V.resize_frames(frame, 4)
    with pytest.raises(ValueError, match="packed uint8 RGB frames"):
        V.resize_frames(frame.astype(np.float32), (4, 4))
    with pytest.raises(ValueError, match="packed uint8 RGB frames"):
        V.resize_frames(frame[..., :2], (4, 4))
    with pytest.raises(ValueError, match="resample= takes one of"):
        V.read_video("nothing.avi", size=(4, 4), resample="nearest")                          # refused before the file is opened


def fake_reader(monkeypatch, n, H=6, W=10):
    """video_io.read_video replaced by one that hands out n numbered host frames and records how it was called"""
    calls = []

    def read_video(path, step=1, length=None, start=0, size=None, resample="bicubic"):
        calls.append(dict(path=path, step=step, length=length, start=start, size=size, resample=resample))
        w, h = size if size is not None else (W, H)
        frames = torch.arange(n, dtype=torch.uint8)[:, None, None, None].expand(n, h, w, 3).contiguous()
        return frames, None, None

    monkeypatch.setattr(V, "read_video", read_video)
    return calls


def frame_numbers(frames):
    assert bool((frames == frames[:, :1, :1, :1]).all())
    return frames[:, 0, 0, 0].tolist()


@pytest.mark.parametrize("n,window,offset,max_length,want,original", [
    (5, 4, 0, None, [0, 1, 2, 3, 4, 4, 4, 4], 5),          # padded with the last frame to two windows
    (8, 4, 0, None, list(range(8)), 8),                    # a whole number of windows: nothing added
    (3, 16, 0, None, [0, 1, 2] + [2] * 13, 3),             # shorter than one window
    (10, 4, 2, 5, [2, 3, 4, 5, 6, 6, 6, 6], 5),            # [offset : offset + max_length], then padded
    (10, 4, 7, 8, [7, 8, 9, 9], 3),                        # the cut runs past the clip's end
    (10, 4, 3, None, list(range(10)) + [9, 9], 10),        # animation.py:178-179: the offset counts only with a max_length
    (10, 1, 0, 4, [0, 1, 2, 3], 4),
])
def test_load_control_clip_cuts_and_pads(monkeypatch, n, window, offset, max_length, want, original):
    calls = fake_reader(monkeypatch, n)
    frames, original_length = V.load_control_clip("pose.avi", (12, 8), window, offset=offset, max_length=max_length, resample="lanczos")
    assert calls == [dict(path="pose.avi", step=1, length=None, start=0, size=(12, 8), resample="lanczos")]
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (len(want), 8, 12, 3)
    assert frame_numbers(frames) == want and original_length == original and len(want) % window == 0


def test_load_control_clip_refusals(monkeypatch):
    fake_reader(monkeypatch, 5)
    with pytest.raises(ValueError, match="selects none"):
        V.load_control_clip("pose.avi", (12, 8), 4, offset=5, max_length=2)
    for kw, msg in ((dict(window=0), "window="), (dict(window=4, offset=-1), "offset="), (dict(window=4, max_length=0), "max_length="),
                    (dict(window=True), "window=")):
        with pytest.raises(ValueError, match=msg):
            V.load_control_clip("pose.avi", (12, 8), **kw)
    with pytest.raises(ValueError, match=r"size=\(width, height\)"):
        V.load_control_clip("pose.avi", 12, 4)
