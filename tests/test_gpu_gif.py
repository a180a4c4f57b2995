"""GPU tests of the GIF writer: emo_gif_histogram / emo_gif_map / emo_gif_lzw_count / emo_gif_lzw_emit (csrc/gif_out.hip) against
tests/gif_ref.py, and the files of encode_gif, the reference surface and `__call__(save_path="clip.gif")` through two decoders, Pillow's and
the helper's own.  Everything is exact: integer histograms, an exact nearest-colour search, and a lossless code - a decoded frame equals
palette[indices] byte for byte, and the device's code streams equal the serial encoder's.

The shapes are the smallest that reach each way the kernels can go: odd sizes with tail lanes and several strips (2x37x53), one pixel,
one bin for every atomic, the largest sums, 8192 random pixels in one strip (the table fills: a Clear inside the strip, all four code
widths), one index (the longest strings), one-pixel strips, and frames whose streams end at different bit phases."""
import io
from fractions import Fraction

import numpy as np
import pytest
import torch
from PIL import Image

from emote_hack_amd import video_io as V
from emote_hack_amd.synth import seeded_randn
from tests import cases
from tests import gif_ref as R
from tests.test_gpu_kernels import DEV, ops

pytestmark = pytest.mark.gpu
POISON = 0xA5


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                                 # a copy: the shared clip is read-only


@pytest.fixture(scope="module")
def clip():
    frames = R.synthetic_clip(2, 37, 53, 3)
    frames[0, 0, :4] = 0                                                         # pixels at both ends of the range, for the dither's clamp
    frames[0, 1, :4] = 255
    frames[1, 36, 49:] = (0, 255, 0)
    frames.setflags(write=False)
    return frames


# ------------------------------------------------------------------------------------------------------------------------------ histogram
def one_colour(n, H, W, rgb):
    a = np.zeros((n, H, W, 3), np.uint8)
    a[...] = rgb
    return a


@pytest.mark.parametrize("name", ["odd", "pixel", "one_bin", "largest_sums"])
def test_histogram_equals_bincount(name, clip):
    frames = {"odd": clip, "pixel": one_colour(1, 1, 1, (9, 200, 31)), "one_bin": one_colour(1, 64, 64, (131, 7, 250)),
              "largest_sums": one_colour(3, 16, 16, (255, 255, 255))}[name]
    o = ops()
    got = o.gif_histogram(dev(frames))
    assert got.dtype == torch.int64 and tuple(got.shape) == (1, 32768, 4)
    assert np.array_equal(got[0].cpu().numpy(), R.histogram(frames)), name
    per = o.gif_histogram(dev(frames), per_frame=True).cpu().numpy()
    assert per.shape == (len(frames), 32768, 4)
    for i, f in enumerate(frames):
        assert np.array_equal(per[i], R.histogram(f)), (name, i)
    if name == "one_bin":
        b = (131 >> 3) << 10 | (7 >> 3) << 5 | (250 >> 3)
        assert got[0, b].tolist() == [4096, 4096 * 131, 4096 * 7, 4096 * 250] and int(got[0, :, 0].sum()) == 4096


def test_histogram_of_a_mixed_frame_with_flat_runs():
    """runs of one bin that start and end inside a lane's eight pixels, inside a wavefront's 512, and across the frame boundary"""
    rng = np.random.default_rng(8)
    frames = rng.integers(0, 256, (3, 23, 61, 3), dtype=np.uint8)
    frames[0, 3:17] = (40, 41, 42)
    frames[1].reshape(-1, 3)[5:1300] = (250, 1, 128)
    frames[1, 22, 50:] = (7, 7, 7)
    frames[2, 0, :9] = (7, 7, 7)                                                 # the same bin on both sides of a frame boundary
    o = ops()
    assert np.array_equal(o.gif_histogram(dev(frames))[0].cpu().numpy(), R.histogram(frames))
    per = o.gif_histogram(dev(frames), per_frame=True).cpu().numpy()
    for i in range(3):
        assert np.array_equal(per[i], R.histogram(frames[i])), i


# ------------------------------------------------------------------------------------------------------------------------------ map
def padded(palette):
    out = np.zeros((256, 3), np.uint8)
    out[:len(palette)] = palette
    return out


def test_map_equals_the_brute_force_search(clip):
    o = ops()
    palette, k = V.median_cut(R.histogram(clip), 256)
    assert k == 256
    got = o.gif_map(dev(clip), dev(padded(palette)[None]), 256)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 37, 53)
    assert np.array_equal(got.cpu().numpy(), R.nearest(clip, palette))
    for k in (1, 2):                                                             # entries behind n_colors are never read: poison them
        pal = np.full((256, 3), 128, np.uint8)
        pal[:k] = palette[:k]
        got = o.gif_map(dev(clip), dev(pal[None]), k).cpu().numpy()
        assert np.array_equal(got, R.nearest(clip, palette[:k])) and int(got.max()) == k - 1


def test_map_ties_go_to_the_lowest_index():
    o = ops()
    # entry 1 repeats entry 3; (10, 10, 10) lies exactly between entries 0 and 2, (30, 10, 10) between entries 2 and 4
    palette = np.array([[0, 10, 10], [200, 200, 200], [20, 10, 10], [200, 200, 200], [40, 10, 10], [20, 10, 10]], np.uint8)
    px = np.array([[10, 10, 10], [30, 10, 10], [200, 200, 200], [201, 199, 200], [20, 10, 10], [10, 11, 10], [255, 255, 255], [0, 0, 0]], np.uint8)
    frames = np.tile(px, (3, 1)).reshape(1, 3, 8, 3)
    want = R.nearest(frames, palette)
    assert want[0, 0].tolist() == [0, 2, 1, 1, 2, 0, 1, 0]
    assert np.array_equal(o.gif_map(dev(frames), dev(padded(palette)[None]), 6).cpu().numpy(), want)


def test_map_with_a_palette_per_frame(clip):
    o = ops()
    pals = np.stack([padded(V.median_cut(R.histogram(f), 64)[0]) for f in clip])
    assert not np.array_equal(pals[0], pals[1])
    got = o.gif_map(dev(clip), dev(pals), 64).cpu().numpy()
    for i in range(2):
        assert np.array_equal(got[i], R.nearest(clip[i], pals[i][:64])), i
    assert not np.array_equal(got[1], R.nearest(clip[1], pals[0][:64]))          # frame 1 did not get frame 0's table


@pytest.mark.parametrize("strength", [1, 32, 128])
def test_map_with_the_ordered_dither(strength):
    o = ops()
    frames = R.synthetic_clip(2, 19, 23, 5)
    frames[0, :2] = 0
    frames[0, 2:4] = 255
    frames[1, :, :3] = (0, 255, 3)
    palette, k = V.median_cut(R.histogram(frames), 32)
    moved = R.dithered(frames, strength)
    assert strength == 1 or not np.array_equal(moved, frames)
    if strength == 128:
        assert int((moved[0, :2] > 0).sum()) > 0 and int((moved[0, 2:4] < 255).sum()) > 0 and int(moved.max()) == 255 and int(moved.min()) == 0
    got = o.gif_map(dev(frames), dev(padded(palette)[None]), k, strength).cpu().numpy()
    assert np.array_equal(got, R.nearest(moved, palette)), strength
    indices, pals, used = V.quantize_frames(dev(frames), 32, dither="bayer", dither_strength=strength)
    assert used == k and np.array_equal(pals[0, :k], palette) and not pals[0, k:].any() and np.array_equal(indices.cpu().numpy(), got)


def test_bayer_matrix_of_the_helper():
    b = R.bayer(8)
    assert sorted(b.reshape(-1).tolist()) == list(range(64)) and b[0, :2].tolist() == [0, 32] and b[1, :2].tolist() == [48, 16]


# ------------------------------------------------------------------------------------------------------------------------------ LZW + file
def check_file(data, want_rgb, delays, loop=0, tables=None, indices=None):
    """both decoders: Pillow's frames and the helper's equal want_rgb (n, H, W, 3) byte for byte; timing, loop flag and framing are right"""
    n, H, W, _ = want_rgb.shape
    im = Image.open(io.BytesIO(data))
    assert getattr(im, "n_frames", 1) == n and im.size == (W, H) and im.info["loop"] == loop
    for i in range(n):
        im.seek(i)
        assert im.info["duration"] == 10 * delays[i], i
        assert np.array_equal(np.asarray(im.convert("RGB")), want_rgb[i]), f"Pillow, frame {i}"
    parsed = R.parse_gif(data)
    assert parsed["trailer"] and parsed["loop"] == loop and (parsed["width"], parsed["height"]) == (W, H) and len(parsed["frames"]) == n
    assert [f["delay"] for f in parsed["frames"]] == list(delays)
    for i, f in enumerate(parsed["frames"]):
        table = parsed["global_table"] if f["table"] is None else f["table"]
        assert table.shape == (256, 3) and (f["width"], f["height"], f["left"], f["top"]) == (W, H, 0, 0) and max(f["sub_blocks"]) <= 255
        assert np.array_equal(table[f["indices"]], want_rgb[i]), f"the helper's decoder, frame {i}"
        if tables is not None:
            assert np.array_equal(table, tables[i if len(tables) > 1 else 0])
        if indices is not None:
            assert np.array_equal(f["indices"], indices[i])
    return parsed


def distinct_palette(seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(256), rng.permutation(256), rng.permutation(256)], axis=1).astype(np.uint8)[None]


def check_streams(indices, strip_rows):
    """gif_code_streams of (n, H, W) indices: the serial encoder's bytes, and a file both decoders turn back into the indices"""
    n, H, W = indices.shape
    out, starts, nbytes = V.gif_code_streams(dev(indices), strip_rows)
    host = out.cpu().numpy()
    streams = [host[s:s + b].tobytes() for s, b in zip(starts, nbytes)]
    for i in range(n):
        ref, bits = R.lzw_encode_strips(indices[i], strip_rows)
        assert int(nbytes[i]) == len(ref) == (bits + 7) // 8 and streams[i] == ref, (strip_rows, i)
    assert not host[int(starts[-1] + nbytes[-1]):].any()
    palette, delays = distinct_palette(n * H + W), V.gif_delays(10, n)
    check_file(V.gif_container(W, H, palette, streams, delays), palette[0][indices], delays, tables=palette, indices=indices)
    return streams


@pytest.mark.parametrize("strip_rows", [1, 8, 5, None])
def test_strips_of_a_quantised_clip(strip_rows, clip):
    indices, _, _ = V.quantize_frames(dev(clip))
    check_streams(indices.cpu().numpy(), strip_rows)


@pytest.mark.parametrize("strip_rows", [None, 64])
def test_a_strip_that_fills_the_table(strip_rows):
    """8192 uniform random indices in one strip: almost every pair is new, so more than 3838 strings are made, the table fills, a Clear
    goes into the strip, and the codes pass 9, 10, 11 and 12 bits"""
    indices = np.random.default_rng(11).integers(0, 256, (1, 64, 128), dtype=np.uint8)
    o = ops()
    codes, n_codes, bits = o.gif_lzw_count(dev(indices), 64)
    assert tuple(n_codes.shape) == (1, 1) and tuple(codes.shape) == (1, 1, 8192 + 8192 // 3839 + 2)
    ne = int(n_codes[0, 0])
    row = codes[0, 0, :ne].cpu().numpy()
    assert ne > 3840 and int(row[3839]) == R.CLEAR and int((row == R.CLEAR).sum()) == ne // 3840 and 2048 <= int(row.max()) < 4096
    streams = check_streams(indices, strip_rows)
    assert len(streams[0]) * 8 - 7 <= int(bits[0, 0]) <= len(streams[0]) * 8


def test_one_index_one_pixel_and_one_pixel_strips():
    flat = np.full((1, 40, 40), 201, np.uint8)
    assert len(check_streams(flat, None)[0]) < 80                                # 1600 pixels in some 56 strings
    check_streams(flat, 8)
    check_streams(np.array([[[7]]], np.uint8), 8)                                # Clear, one code, End of Information
    check_streams(np.random.default_rng(1).integers(0, 256, (2, 9, 1), dtype=np.uint8), 1)      # W = 1: one pixel per strip


def test_frames_that_end_at_different_bit_phases():
    """frames start on bytes, their strips do not: seams inside a byte, and between frames inside a 32-bit word"""
    rng = np.random.default_rng(5)
    indices = rng.integers(0, 4, (3, 5, 7), dtype=np.uint8)
    indices[1, 2:] = 1
    indices[2] = 3
    o = ops()
    _, _, bits = o.gif_lzw_count(dev(indices), 2)
    ends = np.cumsum(bits.cpu().numpy(), axis=1)
    assert len({int(e) % 8 for e in ends[:, -1]}) == 3 and (ends[:, :-1] % 8 != 0).any()
    _, starts, _ = V.gif_code_streams(dev(indices), 2)
    assert any(int(s) % 4 for s in starts)
    check_streams(indices, 2)
    check_streams(indices, None)


def test_emit_touches_nothing_outside_its_streams():
    from emote_hack_amd._lib import EmoHipError
    o = ops()
    indices = dev(np.random.default_rng(2).integers(0, 256, (2, 6, 9), dtype=np.uint8))
    codes, n_codes, bits = o.gif_lzw_count(indices, 4)
    ends = torch.cumsum(bits, dim=1, dtype=torch.int64)
    nbytes = (ends[:, -1].cpu().numpy() + 7) // 8
    starts = torch.tensor([0, int(nbytes[0]) * 8], device=DEV)
    offsets = (ends - bits + starts[:, None]).contiguous()
    total = int(nbytes.sum())
    words = (total + 3) // 4 * 4
    buf = torch.full((words + 64,), POISON, device=DEV, dtype=torch.uint8)
    buf[:total] = 0
    o.gif_lzw_emit(codes, n_codes, offsets, buf[:words], 6, 9, 4)
    host = buf.cpu().numpy()
    assert bool((host[total:] == POISON).all())
    assert host[:nbytes[0]].tobytes() == R.lzw_encode_strips(indices[0].cpu().numpy(), 4)[0]
    fresh = torch.full((64,), POISON, device=DEV, dtype=torch.uint8)             # offsets that point outside the buffer write nothing at all
    o.gif_lzw_emit(codes, n_codes, offsets + 8 * 64, fresh, 6, 9, 4)
    o.gif_lzw_emit(codes, n_codes, offsets - 8 * 4096, fresh, 6, 9, 4)
    assert bool((fresh == POISON).all())
    with pytest.raises(EmoHipError, match="multiple of 4"):
        o.gif_lzw_emit(codes, n_codes, offsets, torch.zeros(30, device=DEV, dtype=torch.uint8), 6, 9, 4)
    with pytest.raises(EmoHipError):
        V.encode_gif(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 25)             # host frames: no CPU path


@pytest.mark.parametrize("palette", ["global", "frame"])
def test_encode_gif_decodes_to_the_nearest_palette_colours(palette, clip):
    frames = dev(clip)
    indices, pals, used = V.quantize_frames(frames, palette=palette)
    host = indices.cpu().numpy()
    assert pals.shape == ((1 if palette == "global" else 2), 256, 3)
    for i in range(2):
        t = pals[i if palette == "frame" else 0]
        k = used[i] if palette == "frame" else used
        assert np.array_equal(t[:k], V.median_cut(R.histogram(clip[i] if palette == "frame" else clip), 256)[0]) and not t[k:].any()
        assert np.array_equal(host[i], R.nearest(clip[i], t[:k]))
    want = np.stack([pals[i if palette == "frame" else 0][host[i]] for i in range(2)])
    data = V.encode_gif(frames, 30, loop=2, palette=palette)
    assert data == V.encode_gif(frames, 30, loop=2, palette=palette)             # the atomics are integer adds and ORs: the same bytes every run
    parsed = check_file(data, want, [3, 4], loop=2, tables=pals, indices=host)
    assert all((f["table"] is None) == (palette == "global") for f in parsed["frames"])
    assert data != V.encode_gif(frames, 30, loop=2, palette=palette, strip_rows=None)
    five = V.encode_gif(frames[None], 30, loop=2, palette=palette)               # the (1, n, H, W, 3) of output_type="uint8"
    assert five == data


def test_frames_with_tables_of_different_sizes():
    """palette="frame" where one frame is flat: its table has one entry, the other's 256, and each frame is mapped to its own"""
    frames = R.synthetic_clip(2, 16, 24, 6)
    frames[1] = (12, 34, 56)
    indices, pals, used = V.quantize_frames(dev(frames), palette="frame")
    assert used[1] == 1 and used[0] > 1 and pals[1, 0].tolist() == [12, 34, 56] and not pals[1, 1:].any() and not indices[1].any()
    assert np.array_equal(indices[0].cpu().numpy(), R.nearest(frames[0], pals[0, :used[0]]))
    want = np.stack([pals[i][indices[i].cpu().numpy()] for i in range(2)])
    check_file(V.encode_gif(dev(frames), 25, palette="frame"), want, [4, 4], tables=pals)


# ------------------------------------------------------------------------------------------------------------------------------ surface
def quantised(frames_u8, **kw):
    indices, pals, _ = V.quantize_frames(frames_u8, **kw)
    host = indices.cpu().numpy()
    return np.stack([pals[i if len(pals) > 1 else 0][host[i]] for i in range(len(host))])


def test_reference_surface_writes_gifs(tmp_path):
    videos = torch.rand(3, 3, 4, 10, 6, generator=torch.Generator().manual_seed(3))
    path = tmp_path / "sub" / "grid.gif"                                         # the directory is made (util.py:32)
    V.save_videos_grid(videos, str(path), n_rows=2, fps=8, format="gif", loop=1)
    grid = V.make_grid_u8(videos.to(DEV), n_rows=2)
    assert tuple(grid.shape) == (4, 26, 18, 3)
    check_file(path.read_bytes(), quantised(grid), V.gif_delays(8, 4), loop=1)
    path2 = tmp_path / "frames.gif"
    V.images2video([f for f in grid.cpu().numpy()], str(path2), format="gif", colors=16, strip_rows=3)
    want = quantised(grid, colors=16)
    assert len(np.unique(want.reshape(-1, 3), axis=0)) <= 16
    check_file(path2.read_bytes(), want, V.gif_delays(8, 4))                     # images2video's default rate
    path3 = tmp_path / "direct.gif"
    V.write_video(grid, path3, 8, format="gif", loop=1)
    assert path3.read_bytes() == path.read_bytes()


F_TOT = 4
LOOP_KW = dict(num_inference_steps=2, guidance_scale=7.5, context_frames=4, context_stride=1, context_overlap=0, seed=0)


@pytest.fixture(scope="module")
def env():
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    from tests.test_gpu_unet import build
    from tests.test_gpu_vae import SMALL, build as build_vae
    e = {}
    e["ref"] = build(cases.TINY, torch.float32, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    e["vae"] = build_vae(SMALL, torch.float32)[0]
    e["pipe"] = EMOAnimationPipeline(vae=e["vae"], unet=build(cases.TINY_MOTION, torch.float32), scheduler=DDIMScheduler())
    e["kw"] = dict(video_length=F_TOT, height=128, width=128, latents=seeded_randn((1, 4, F_TOT, 16, 16), 5).to(DEV),
                   text_embeddings=seeded_randn((2, 5, 32), 2), ref_image_latents=seeded_randn((1, 4, 16, 16), 3), appearance_encoder=e["ref"],
                   audio_features=seeded_randn((F_TOT, 5, 32), 7), **LOOP_KW)
    return e


def test_call_save_path_writes_a_gif(env, tmp_path, monkeypatch):
    pipe, kw = env["pipe"], env["kw"]
    path = tmp_path / "clip.gif"
    plain = pipe("", output_type="uint8", **kw).videos
    got = pipe("", output_type="uint8", fps=8, save_path=str(path), **kw).videos
    assert torch.equal(got, plain) and tuple(got.shape) == (1, F_TOT, 128, 128, 3)      # the return value is what it is without save_path
    delays = V.gif_delays(8, F_TOT)
    assert sum(delays) == 50
    check_file(path.read_bytes(), quantised(got[0]), delays, loop=0)
    assert path.read_bytes() == V.encode_gif(got, 8)
    # interpolated frames halve the delays; the options reach the writer; audio drives nothing in the file
    path2 = tmp_path / "clip2.gif"
    samples = np.zeros(16000, np.float32)
    twice = pipe("", output_type="uint8", interpolation_factor=2, fps=8, audio=(samples, 16000), save_path=path2, save_palette="frame",
                 save_dither="bayer", save_dither_strength=16, save_loop=3, **kw).videos
    n_frames = (F_TOT - 1) * 2 + 1
    assert tuple(twice.shape) == (1, n_frames, 128, 128, 3)
    halved = V.gif_delays(16, n_frames)
    assert sum(halved) == int(Fraction(100 * n_frames, 16) + Fraction(1, 2)) and max(halved) == 7 and min(halved) == 6 and min(delays) == 12
    check_file(path2.read_bytes(), quantised(twice[0], palette="frame", dither="bayer", dither_strength=16), halved, loop=3)
    # an `.avi` path still goes the way it went: the same bytes, and none of the GIF kernels
    o = ops()

    def never(*a, **k):
        raise AssertionError("a GIF kernel on the way to an `.avi` file")
    for name in ("gif_histogram", "gif_map", "gif_lzw_count", "gif_lzw_emit"):
        monkeypatch.setattr(o, name, never)
    path3 = tmp_path / "clip.avi"
    again = pipe("", output_type="uint8", fps=8, save_path=str(path3), **kw).videos
    jpegs, fps, audio = V.read_avi(path3)
    assert torch.equal(again, plain) and fps == 8 and audio is None and jpegs == V.encode_mjpeg(plain, 90)
