"""Host tests of the GIF writer (emote_hack_amd/video_io.py): frame delays, the median cut measured against Pillow's, the container around
streams from the serial encoder of tests/gif_ref.py, and every refusal that comes before a launch.  No GPU.

Quality bar: the PSNR of palette[nearest] is at least that of Pillow's `quantize(256, method=MEDIANCUT, dither=NONE)` on the same frames
stacked into one image - Pillow is the reference, the bar has no margin."""
import io
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from emote_hack_amd import video_io as V
from tests import gif_ref as R

CLIPS = ((1, 64, 64), (3, 96, 80), (2, 128, 128))


def test_gif_delays_keep_the_duration():
    assert V.gif_delays(25, 7) == [4] * 7
    d30 = V.gif_delays(30, 30)
    assert sum(d30) == 100 and set(d30) == {3, 4} and d30[:3] == [3, 4, 3]       # 3.33 cs per frame: halves round up, the sum is exact
    ntsc = V.gif_delays(Fraction(30000, 1001), 300)
    assert sum(ntsc) == 1001 and set(ntsc) == {3, 4}                             # 300 frames last 10.01 s
    assert V.gif_delays((25, 2), 2) == [8, 8] and V.gif_delays(50, 3) == [2, 2, 2] and V.gif_delays(1, 1) == [100]
    for bad, n in ((60, 4), (60, 2), (51, 60), (Fraction(101, 2), 200)):          # a delay of 1 turns up sooner or later
        with pytest.raises(ValueError, match="50 frames per second"):
            V.gif_delays(bad, n)
    for bad in (0, -3, 2.5, "25", (25,), True):
        with pytest.raises(ValueError, match="fps"):
            V.gif_delays(bad, 4)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="frames"):
            V.gif_delays(25, bad)
    with pytest.raises(ValueError, match="65535"):
        V.gif_delays(Fraction(1, 700), 1)


@pytest.mark.parametrize("n,H,W", CLIPS)
def test_median_cut_is_no_worse_than_pillows(n, H, W):
    clip = R.synthetic_clip(n, H, W, 1)
    hist = R.histogram(clip)
    palette, k = V.median_cut(hist, 256)
    assert palette.dtype == np.uint8 and palette.shape == (k, 3) and 2 <= k <= 256
    again, k2 = V.median_cut(hist.copy(), 256)
    assert k2 == k and np.array_equal(again, palette)                            # deterministic
    stacked = clip.reshape(n * H, W, 3)
    theirs = np.asarray(Image.fromarray(stacked).quantize(256, method=Image.Quantize.MEDIANCUT, dither=Image.Dither.NONE).convert("RGB"))
    mine, pillow = R.psnr(palette[R.nearest(clip, palette)], clip), R.psnr(theirs, stacked)
    print(f"{n}x{H}x{W}: k = {k}, median_cut {mine:.2f} dB, Pillow MEDIANCUT {pillow:.2f} dB")
    assert mine >= pillow
    small, ks = V.median_cut(hist, 16)
    assert ks == 16 and R.psnr(small[R.nearest(clip, small)], clip) < mine


def test_median_cut_on_degenerate_histograms():
    one = np.full((5, 7, 3), 0, np.uint8)
    one[...] = (201, 13, 77)
    pal, k = V.median_cut(R.histogram(one), 256)
    assert k == 1 and pal.tolist() == [[201, 13, 77]]
    two = one.copy()
    two[:2] = (10, 250, 77)
    pal, k = V.median_cut(R.histogram(two), 256)
    assert k == 2 and sorted(pal.tolist()) == [[10, 250, 77], [201, 13, 77]]
    pal2, k2 = V.median_cut(R.histogram(two), 2)
    assert k2 == 2 and np.array_equal(pal2, pal)
    # two colours in ONE bin cannot be told apart: one entry, their mean rounded half up
    near = one.copy()
    near[0, 0] = (202, 14, 78)
    near[0, 1] = (202, 14, 78)
    pal, k = V.median_cut(R.histogram(near), 256)
    mean = (2 * near.reshape(-1, 3).astype(np.int64).sum(0) + 35) // 70
    assert k == 1 and pal[0].tolist() == mean.tolist()
    # 100 occupied bins, 256 asked for: every bin gets its own entry, the mean of its pixels
    rng = np.random.default_rng(4)
    bins = rng.choice(32768, 100, replace=False)
    base = np.stack([(bins >> 10) << 3, ((bins >> 5) & 31) << 3, (bins & 31) << 3], axis=1)
    px = (base[rng.integers(0, 100, 4000)] + rng.integers(0, 8, (4000, 3))).astype(np.uint8)
    hist = R.histogram(px)
    pal, k = V.median_cut(hist, 256)
    occ = np.flatnonzero(hist[:, 0])
    want = (2 * hist[occ, 1:] + hist[occ, :1]) // (2 * hist[occ, :1])
    assert k == len(occ) <= 100 and sorted(pal.tolist()) == sorted(want.tolist())
    pal, k = V.median_cut(hist, 2)
    assert k == 2
    for bad in (1, 0, 257, 2.0, True, None):
        with pytest.raises(ValueError, match="colors="):
            V.median_cut(hist, bad)
    with pytest.raises(ValueError, match="no pixels"):
        V.median_cut(np.zeros((32768, 4), np.int64))
    with pytest.raises(ValueError, match="32768"):
        V.median_cut(np.zeros((32768, 3), np.int64))


def test_container_frames_what_the_reference_encoder_codes():
    rng = np.random.default_rng(2)
    H, W, delays = 37, 53, [3, 4, 3]
    palettes = rng.integers(0, 256, (3, 256, 3), dtype=np.uint8)
    indices = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    indices[1, 5:30] = 9                                                         # a flat band: long strings
    for strip_rows, pals in ((8, palettes[:1]), (None, palettes), (1, palettes)):
        streams = [R.lzw_encode_strips(f, strip_rows)[0] for f in indices]
        data = V.gif_container(W, H, pals, streams, delays, loop=5)
        assert data[:6] == b"GIF89a" and data[-1:] == b"\x3B"
        im = Image.open(io.BytesIO(data))
        assert im.n_frames == 3 and im.size == (W, H) and im.info["loop"] == 5
        for i in range(3):
            im.seek(i)
            assert im.info["duration"] == 10 * delays[i]
            assert np.array_equal(np.asarray(im.convert("RGB")), pals[i if len(pals) > 1 else 0][indices[i]]), (strip_rows, i)
        parsed = R.parse_gif(data)
        assert parsed["trailer"] and parsed["loop"] == 5 and (parsed["width"], parsed["height"]) == (W, H) and len(parsed["frames"]) == 3
        assert np.array_equal(parsed["global_table"], pals[0])
        for i, f in enumerate(parsed["frames"]):
            assert f["delay"] == delays[i] and f["disposal"] == 1 and f["transparent"] is None and f["code_size"] == 8
            assert (f["left"], f["top"], f["width"], f["height"]) == (0, 0, W, H)
            assert max(f["sub_blocks"]) <= 255 and all(s == 255 for s in f["sub_blocks"][:-1]) and f["stream"] == streams[i]
            assert (f["table"] is None) == (len(pals) == 1) and (f["table"] is None or np.array_equal(f["table"], pals[i]))
            assert np.array_equal(f["indices"], indices[i])
    assert V.gif_sub_blocks(b"") == b"\x00" and V.gif_sub_blocks(bytes(255)) == b"\xFF" + bytes(255) + b"\x00"
    assert V.gif_sub_blocks(bytes(256)) == b"\xFF" + bytes(255) + b"\x01\x00\x00"
    one = [streams[0]]
    for bad in (-1, 65536, 1.0, True):
        with pytest.raises(ValueError, match="loop="):
            V.gif_container(W, H, palettes[:1], one, [4], loop=bad)
    for w, h in ((0, 5), (5, 0), (65536, 5), (5, 65536)):
        with pytest.raises(ValueError, match="65535"):
            V.gif_container(w, h, palettes[:1], one, [4])
    with pytest.raises(ValueError, match="delays"):
        V.gif_container(W, H, palettes[:1], one, [4, 4])
    with pytest.raises(ValueError, match="colour tables"):
        V.gif_container(W, H, palettes[:2], [streams[0]] * 3, [4] * 3)


def test_gif_refusals_come_before_any_launch(tmp_path):
    """host tensors: a launch would raise EmoHipError, so every ValueError here was raised before one"""
    frames = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    good = str(tmp_path / "clip.gif")
    for kw, match in ((dict(colors=1), "colors="), (dict(colors=257), "colors="), (dict(colors=16.0), "colors="), (dict(loop=-1), "loop="),
                      (dict(loop=65536), "loop="), (dict(strip_rows=0), "strip_rows="), (dict(strip_rows=2.5), "strip_rows="),
                      (dict(strip_rows=True), "strip_rows="), (dict(palette="local"), "palette="), (dict(dither="floyd"), "dither="),
                      (dict(dither="bayer", dither_strength=0), "dither_strength="), (dict(dither_strength=129), "dither_strength=")):
        with pytest.raises(ValueError, match=match):
            V.encode_gif(frames, 25, **kw)
        with pytest.raises(ValueError, match=match):
            V.write_video(frames, good, 25, format="gif", **kw)
    with pytest.raises(ValueError, match="50 frames per second"):
        V.encode_gif(frames, 60)
    for bad in (frames.float(), torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 8, 4, dtype=torch.uint8), np.zeros((1, 8, 8, 3), np.uint8)):
        with pytest.raises(ValueError, match="uint8 RGB frames"):
            V.encode_gif(bad, 25)
    with pytest.raises(ValueError, match="no frames"):
        V.encode_gif(torch.zeros(0, 8, 8, 3, dtype=torch.uint8), 25)
    with pytest.raises(ValueError, match="65535"):
        V.encode_gif(torch.zeros(1, 1, 65536, 3, dtype=torch.uint8), 25)
    with pytest.raises(ValueError, match=r"\.gif"):
        V.write_gif(frames, tmp_path / "clip.avi", 25)
    with pytest.raises(ValueError, match="unknown option"):
        V.write_gif(frames, good, 25, quality=90)
    videos = torch.rand(1, 3, 2, 8, 8)
    stills = [np.zeros((8, 8, 3), np.uint8)]
    for bad in ("GIF", "avi", "mp4", 1, True):
        with pytest.raises(ValueError, match="format="):
            V.write_video(frames, good, 25, format=bad)
        with pytest.raises(ValueError, match="format="):
            V.save_videos_grid(videos, good, format=bad)
        with pytest.raises(ValueError, match="format="):
            V.images2video(stills, good, format=bad)
    for name in ("clip.avi", "clip.mp4", "clip", "clip.gif.avi"):
        with pytest.raises(ValueError, match=r"\.gif"):
            V.write_video(frames, tmp_path / name, 25, format="gif")
        with pytest.raises(ValueError, match=r"\.gif"):
            V.save_videos_grid(videos, str(tmp_path / name), format="gif")
        with pytest.raises(ValueError, match=r"\.gif"):
            V.images2video(stills, str(tmp_path / name), format="gif")
    for kw in (dict(quality=50), dict(restart_interval="row"), dict(restart_interval=4)):
        with pytest.raises(ValueError, match="quality= and restart_interval="):
            V.write_video(frames, good, 25, format="gif", **kw)
        with pytest.raises(ValueError, match="quality= and restart_interval="):
            V.save_videos_grid(videos, good, format="gif", **kw)
        with pytest.raises(ValueError, match="quality= and restart_interval="):
            V.images2video(stills, good, format="gif", **kw)
    with pytest.raises(ValueError, match="no sound"):
        V.write_video(frames, good, 25, format="gif", audio=(np.zeros(100, np.float32), 16000))
    with pytest.raises(ValueError, match="unknown option"):
        V.write_video(frames, good, 25, format="gif", colours=16)
    assert list(tmp_path.iterdir()) == []


def test_without_the_keyword_nothing_changes(tmp_path):
    frames = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    for name in ("clip.gif", "clip.mp4"):
        with pytest.raises(ValueError, match=r"\.avi") as e:
            V.write_video(frames, tmp_path / name, 25)
        assert "format=\"gif\"" in str(e.value) and "gif need" not in str(e.value)       # the way to a GIF, not a claim that there is none
        with pytest.raises(ValueError, match=r"\.avi"):
            V.save_videos_grid(torch.rand(1, 3, 2, 8, 8), str(tmp_path / name))
        with pytest.raises(ValueError, match=r"\.avi"):
            V.images2video([np.zeros((8, 8, 3), np.uint8)], str(tmp_path / name))
    for kw in (dict(loop=1), dict(colors=16), dict(strip_rows=4)):                # GIF options without format="gif"
        with pytest.raises(ValueError, match="format=\"gif\""):
            V.write_video(frames, tmp_path / "clip.avi", 25, **kw)
    assert list(tmp_path.iterdir()) == []


def test_call_save_path_gif_refusals(tmp_path):
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    p = EMOAnimationPipeline(unet=SimpleNamespace(device=torch.device("cpu")), scheduler=DDIMScheduler())      # no VAE
    good = str(tmp_path / "clip.gif")
    with pytest.raises(ValueError, match="fps="):
        p("", 2, save_path=good)
    with pytest.raises(ValueError, match="VAE"):
        p("", 2, save_path=good, fps=8)                                          # a `.gif` path is taken; the checks go on to the next one
    with pytest.raises(ValueError, match=r"\.avi"):
        p("", 2, save_path=str(tmp_path / "clip.mp4"), fps=8)
    for kw, match in ((dict(save_restart_interval="row"), "save_restart_interval="), (dict(save_quality=50), "save_quality="),
                      (dict(save_palette="local"), "palette="), (dict(save_dither="floyd"), "dither="),
                      (dict(save_dither="bayer", save_dither_strength=200), "dither_strength="), (dict(save_loop=-1), "save_loop=")):
        with pytest.raises(ValueError, match=match):
            p("", 2, save_path=good, fps=8, **kw)
    with pytest.raises(ValueError, match="50 frames per second"):
        p("", 2, save_path=good, fps=60)
    with pytest.raises(ValueError, match="50 frames per second"):
        p("", 2, save_path=good, fps=30, interpolation_factor=2)                 # the file plays at fps * interpolation_factor
    with pytest.raises(ValueError, match=r"`\.gif` save_path"):
        p("", 2, save_path=str(tmp_path / "clip.avi"), fps=8, save_loop=3)
    assert list(tmp_path.iterdir()) == []
