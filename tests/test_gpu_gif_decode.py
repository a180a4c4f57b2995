"""GPU tests of the GIF reader: emo_gif_lzw_decode and emo_gif_compose (csrc/gif_in.hip) against the numpy reference of
tests/gif_decode_ref.py - which tests/test_gif_decode_host.py holds against Pillow on the same cases - and decode_gif / read_image /
read_video / load_control_clip / video2images / controlnet_condition= against Pillow and against this project's own writer.  Every
comparison is byte for byte.

The stream buffer and the indices lie inside larger buffers filled with a guard byte, which every kernel-level test checks: a damaged
stream gives a status, and nothing outside the frame's own bytes is written."""
import functools
import io
from fractions import Fraction

import numpy as np
import pytest
import torch
from PIL import Image

from emote_hack_amd import ops
from emote_hack_amd import video_io as V
from emote_hack_amd._lib import EmoHipError
from emote_hack_amd.synth import seeded_randn
from tests import cases
from tests import gif_decode_cases as K
from tests import gif_decode_ref as R
from tests import gif_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, POISON = 256, 0xA5


def lzw(streams, code_sizes, pixels):
    """one launch over the streams -> (indices as bytes per frame, produced, status); streams and indices lie between guard bytes"""
    n = len(streams)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    out_offsets = np.concatenate([[0], np.cumsum(pixels)]).astype(np.int64)
    pad = -int(offsets[-1]) % 4 or (4 if offsets[-1] == 0 else 0)
    size, total = int(offsets[-1]) + pad, int(out_offsets[-1])
    host = np.full(size + 2 * GUARD, POISON, np.uint8)                           # what lies around the frames is not zeros
    host[GUARD:GUARD + int(offsets[-1])] = np.frombuffer(b"".join(streams), np.uint8)
    buf = torch.from_numpy(host).to(DEV)
    whole = torch.full((total + 2 * GUARD,), POISON, dtype=torch.uint8, device=DEV)
    code = np.array(code_sizes, np.int32)
    indices, produced, status = ops.gif_lzw_decode(buf[GUARD:GUARD + size], torch.from_numpy(offsets).to(DEV), torch.from_numpy(code).to(DEV),
                                                   torch.from_numpy(out_offsets).to(DEV), total, layout=(offsets, code, out_offsets),
                                                   out=whole[GUARD:GUARD + total])
    torch.cuda.synchronize()
    got, after = whole.cpu().numpy(), buf.cpu().numpy()
    assert (got[:GUARD] == POISON).all() and (got[GUARD + total:] == POISON).all(), "emo_gif_lzw_decode wrote outside indices"
    assert np.array_equal(after, host), "emo_gif_lzw_decode wrote into the streams"
    body = got[GUARD:GUARD + total]
    return [body[a:b].tobytes() for a, b in zip(out_offsets, out_offsets[1:])], produced.cpu().numpy().tolist(), status.cpu().numpy().tolist()


# ------------------------------------------------------------------------------------------------------------------------------ LZW
@pytest.mark.parametrize("name", sorted(K.valid_streams()))
def test_lzw_equals_the_reference(name):
    indices, cs, data, _ = K.valid_streams()[name]
    got, produced, status = lzw([data], [cs], [indices.size])
    assert status == [R.OK] and produced == [indices.size]
    assert got[0] == indices.tobytes()


def test_streams_of_different_lengths_and_code_sizes_share_a_launch():
    s = K.valid_streams()
    names = sorted(s)
    got, produced, status = lzw([s[k][2] for k in names], [s[k][1] for k in names], [s[k][0].size for k in names])
    assert len({len(s[k][2]) for k in names}) > 10 and len({s[k][1] for k in names}) >= 5
    assert status == [R.OK] * len(names) and produced == [s[k][0].size for k in names]
    for k, g in zip(names, got):
        assert g == s[k][0].tobytes(), k
    data, W, H, frames, table, _ = K.built("six_rectangles")
    p = V.parse_gif(data)
    got, produced, status = lzw([f.data for f in p.frames], [f.code_size for f in p.frames], [f.width * f.height for f in p.frames])
    assert status == [R.OK] * 6 and [g for g in got] == [f["indices"].tobytes() for f in frames]


@pytest.mark.parametrize("name", sorted(K.damaged_streams()))
def test_damaged_stream_gives_its_status_and_its_neighbours_decode(name):
    n, cs, data, status, produced, _, want = K.damaged_streams()[name]
    s = K.valid_streams()
    left, right = s["no_leading_clear"], s["cs3_waves"]
    got, made, st = lzw([left[2], data, right[2]], [left[1], cs, right[1]], [left[0].size, n, right[0].size])
    assert st == [R.OK, status, R.OK] and made == [left[0].size, produced, right[0].size]
    assert got[0] == left[0].tobytes() and got[2] == right[0].tobytes()
    assert got[1][:produced] == want and got[1][produced:] == bytes([POISON]) * (n - produced)      # nothing behind what it produced


def test_entries_refuse_bad_shapes_before_any_launch():
    z8 = torch.zeros(8, dtype=torch.uint8, device=DEV)
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64, device=DEV)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=DEV)
    with pytest.raises(EmoHipError, match="multiple of 4"):
        ops.gif_lzw_decode(z8[:6], i64(0, 6), i32(8), i64(0, 4), 4)
    with pytest.raises(EmoHipError, match="code size of 9"):
        ops.gif_lzw_decode(z8, i64(0, 8), i32(9), i64(0, 4), 4, layout=([0, 8], [9], [0, 4]))
    with pytest.raises(EmoHipError, match="total=0"):
        ops.gif_lzw_decode(z8, i64(0, 8), i32(8), i64(0, 0), 0)
    desc, tables = torch.zeros(1, ops.GIF_FRAME_INTS, dtype=torch.int32, device=DEV), torch.zeros(1, 256, 3, dtype=torch.uint8, device=DEV)
    for n_out, H, W in ((0, 2, 2), (2, 2, 2), (1, 0, 2), (1, 2, 65536)):
        with pytest.raises(EmoHipError, match="emo_gif_compose"):
            ops.gif_compose(z8[:4], i64(0, 4), desc, tables, n_out, H, W)
    bad_cs = ops.gif_lzw_decode(z8, i64(0, 8), i32(11), i64(0, 4), 4)
    backwards = ops.gif_lzw_decode(z8, i64(8, 0), i32(8), i64(0, 4), 4)         # a code size and offsets the kernel itself turns down
    assert bad_cs[1].tolist() == [0] and bad_cs[2].tolist() == [R.BAD_CODE] and backwards[1].tolist() == [0] and backwards[2].tolist() == [R.PAST_END]


# ------------------------------------------------------------------------------------------------------------------------------ compose
def compose_on_device(data, slots=None):
    """a file's frames through the reference LZW decoder and emo_gif_compose -> (rgb, status)"""
    p = V.parse_gif(data)
    n = len(p.frames)
    indices = [R.lzw_decode(f.data, f.code_size, f.width * f.height)[0] for f in p.frames]
    out_offsets = np.concatenate([[0], np.cumsum([len(i) for i in indices])]).astype(np.int64)
    slots = {k: k for k in range(n)} if slots is None else slots
    whole = torch.full((len(slots) * p.height * p.width * 3 + 2 * GUARD,), POISON, dtype=torch.uint8, device=DEV)
    rgb, status = ops.gif_compose(torch.from_numpy(np.frombuffer(b"".join(indices), np.uint8).copy()).to(DEV), torch.from_numpy(out_offsets).to(DEV),
                                  torch.from_numpy(V.gif_descriptors(p.frames, slots)).to(DEV), torch.from_numpy(p.tables).to(DEV), len(slots),
                                  p.height, p.width, out=whole[GUARD:-GUARD].view(len(slots), p.height, p.width, 3))
    torch.cuda.synchronize()
    host = whole.cpu().numpy()
    assert (host[:GUARD] == POISON).all() and (host[-GUARD:] == POISON).all(), "emo_gif_compose wrote outside rgb"
    return rgb.cpu().numpy(), status.cpu().numpy().tolist()


def test_compose_equals_the_reference_on_the_random_batch():
    for seed in K.RANDOM_SEEDS:
        data, W, H, frames, table, background = K.random_file(seed)
        got, status = compose_on_device(data)
        assert status == [R.OK] * len(frames), seed
        assert np.array_equal(got, R.compose(W, H, frames, table, background)), seed


@pytest.mark.parametrize("name", K.BUILT)
def test_compose_equals_the_reference_on_built_files(name):
    data, W, H, frames, table, background = K.built(name)
    got, status = compose_on_device(data)
    assert status == [R.OK] * len(frames) and np.array_equal(got, R.compose(W, H, frames, table, background))


def test_compose_returns_only_the_slots_asked_for():
    data, W, H, frames, table, background = K.built("dependent")
    want = R.compose(W, H, frames, table, background)
    got, status = compose_on_device(data, {5: 0, 2: 1})
    assert status == [R.OK] * len(frames) and np.array_equal(got, want[[5, 2]])


def test_compose_flags_an_index_beyond_its_table():
    data, frames = K.bad_index_file()
    got, status = compose_on_device(data)
    assert status == [R.OK, R.BAD_INDEX, R.OK]
    with pytest.raises(ValueError, match=r"frame 1 does not decode: a colour index at or beyond.*emo_gif_compose status 4"):
        V.decode_gif(data)


# ------------------------------------------------------------------------------------------------------------------------------ decode_gif
@pytest.mark.parametrize("name", sorted(K.pillow_files()))
def test_decode_gif_equals_pillow_on_pillow_files(name):
    data = K.pillow_files()[name]
    frames, delays, loop = V.decode_gif(data)
    im = Image.open(io.BytesIO(data))
    assert frames.is_cuda and frames.dtype == torch.uint8 and np.array_equal(frames.cpu().numpy(), R.pillow_frames(data))
    assert loop == im.info.get("loop")
    for k, d in enumerate(delays):
        im.seek(k)
        assert d * 1000 == im.info.get("duration", 0)


@pytest.mark.parametrize("name", K.BUILT)
def test_decode_gif_equals_pillow_on_built_files(name):
    data = K.built(name)[0]
    assert np.array_equal(V.decode_gif(data)[0].cpu().numpy(), R.pillow_frames(data))


def test_decode_gif_equals_pillow_on_stream_cases_and_random_files():
    for name, (indices, cs, stream, _) in K.valid_streams().items():
        table = K.palette(max(1 << cs, 4), cs)
        data = R.build(indices.shape[1], indices.shape[0], [R.frame(indices, code_size=cs, data=stream)], table)
        assert np.array_equal(V.decode_gif(data)[0].cpu().numpy(), R.pillow_frames(data)), name
    for seed in K.RANDOM_SEEDS[:16]:
        data = K.random_file(seed)[0]
        assert np.array_equal(V.decode_gif(data)[0].cpu().numpy(), R.pillow_frames(data)), seed


def test_select_returns_frames_that_depend_on_their_predecessors():
    data = K.built("dependent")[0]
    want = R.pillow_frames(data)
    frames, delays, loop = V.decode_gif(data, select=slice(2, None, 2))
    assert np.array_equal(frames.cpu().numpy(), want[2::2]) and delays == [Fraction(4, 100), Fraction(4, 100), Fraction(4, 100)] and loop == 0
    assert not np.array_equal(want[4], want[2]) and len(want) == 7
    assert np.array_equal(V.decode_gif(data, select=slice(3, 4))[0].cpu().numpy(), want[3:4])
    assert np.array_equal(V.decode_gif(data, select=slice(None, None, -3))[0].cpu().numpy(), want[::-3])
    with pytest.raises(ValueError, match="selects none"):
        V.decode_gif(data, select=slice(7, None))


def test_decode_gif_names_the_frame_the_status_and_how_far_it_got():
    n, cs, stream, *_ = K.damaged_streams()["short_with_eoi"]
    good = R.frame(K.waves(31, 45, 256))
    data = R.build(45, 31, [good, R.frame(np.zeros((31, 45), np.uint8), data=stream, delay=1), good], K.palette(256))
    with pytest.raises(ValueError, match=rf"decode_gif: frame 1 does not decode: End of Information before.*after {17 * 45} of {31 * 45} colour indices"):
        V.decode_gif(data)
    assert V.decode_gif(data, select=slice(0, 1))[0].shape == (1, 31, 45, 3)     # frames behind the last selected one are not decoded


# ------------------------------------------------------------------------------------------------------------------------------ round trip
@functools.lru_cache(None)
def clip():
    return torch.from_numpy(gif_ref.synthetic_clip(5, 40, 56, 3)).to(DEV)


@pytest.mark.parametrize("palette", ["global", "frame"])
@pytest.mark.parametrize("strip_rows", [8, None])
def test_round_trip_through_encode_gif(palette, strip_rows):
    frames = clip()
    indices, palettes, _ = V.quantize_frames(frames, palette=palette)
    want = np.stack([palettes[k if palette == "frame" else 0][indices[k].cpu().numpy()] for k in range(5)])
    data = V.encode_gif(frames, 30, loop=4, palette=palette, strip_rows=strip_rows)
    got, delays, loop = V.decode_gif(data)
    assert np.array_equal(got.cpu().numpy(), want)
    assert [d * 100 for d in delays] == V.gif_delays(30, 5) and loop == 4


def test_own_writer_layout_built_on_the_host():
    for name, (data, indices, palettes, delays, loop) in K.own_writer_files().items():
        got, got_delays, got_loop = V.decode_gif(data)
        want = np.stack([palettes[k if len(palettes) > 1 else 0][indices[k]] for k in range(len(indices))])
        assert np.array_equal(got.cpu().numpy(), want) and [d * 100 for d in got_delays] == delays and got_loop == loop, name


# ------------------------------------------------------------------------------------------------------------------------------ surface
def test_read_video_image_control_clip_and_video2images_take_a_gif(tmp_path):
    frames = clip()
    path = str(tmp_path / "clip.gif")
    V.write_gif(frames, path, 30)
    with open(path, "rb") as f:
        data = f.read()
    want = R.pillow_frames(data)
    got, fps, audio = V.read_video(path)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want) and audio is None
    assert fps == Fraction(500, 17)                                              # 5 frames at 30 fps are written as 3, 4, 3, 3, 4 centiseconds
    got, fps, _ = V.read_video(path, step=2, length=2, start=1)
    assert np.array_equal(got.cpu().numpy(), want[1::2][:2]) and fps == Fraction(500, 17)      # the rate is the file's, whatever is selected
    twelve = str(tmp_path / "twelve.gif")
    V.write_gif(frames[[0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3]], twelve, 30)
    assert V.read_video(twelve, length=1)[1] == 30                               # 12 frames at 30 fps: 40 centiseconds
    small, _, _ = V.read_video(path, size=(28, 20))
    assert np.array_equal(small.cpu().numpy(), np.stack([np.asarray(Image.fromarray(f).resize((28, 20), Image.BICUBIC)) for f in want]))
    with pytest.raises(ValueError, match="selects none"):
        V.read_video(path, start=5)
    for source in (path, data):
        still = V.read_image(source)
        assert still.is_cuda and np.array_equal(still.cpu().numpy(), want[0])
    assert np.array_equal(V.read_image(data, size=(28, 20)).cpu().numpy(), np.asarray(Image.fromarray(want[0]).resize((28, 20), Image.BICUBIC)))
    padded, original = V.load_control_clip(path, (56, 40), 4)
    assert original == 5 and tuple(padded.shape) == (8, 40, 56, 3)
    assert np.array_equal(padded[:5].cpu().numpy(), want) and all(np.array_equal(padded[k].cpu().numpy(), want[4]) for k in (5, 6, 7))
    stills = V.video2images(path, step=2, length=2)
    assert len(stills) == 2 and np.array_equal(np.stack(stills), want[::2][:2])
    mixed = str(tmp_path / "mixed.gif")
    with open(mixed, "wb") as f:
        f.write(K.built("dependent")[0])
    assert V.read_video(mixed, length=1)[1] == Fraction(700, 31)                 # delays of 4 and 5: 4 + 3 * (5 + 4) centiseconds over 7 frames
    uneven = str(tmp_path / "uneven.gif")
    with open(uneven, "wb") as f:
        f.write(R.build(4, 4, [R.frame(K.noise(4, 4, 4, k), delay=d) for k, d in enumerate((3, 5, 3))], K.palette(4)))
    got, fps, _ = V.read_video(uneven)
    assert fps is None and tuple(got.shape) == (3, 4, 4, 3)
    (tmp_path / "empty.gif").write_bytes(R.build(4, 4, [], K.palette(4)))
    with pytest.raises(ValueError, match="read_video: .*no image"):
        V.read_video(str(tmp_path / "empty.gif"))


F_TOT = 4
LOOP_KW = dict(num_inference_steps=2, guidance_scale=7.5, context_frames=4, context_stride=1, context_overlap=0, seed=0, output_type="latent")


def test_control_frames_from_a_gif_reach_the_loop(tmp_path):
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    from tests.test_gpu_controlnet import build_controlnet
    from tests.test_gpu_unet import build
    from tests.test_gpu_vae import SMALL, build as build_vae
    ref = build(cases.TINY, torch.float32, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    pipe = EMOAnimationPipeline(vae=build_vae(SMALL, torch.float32)[0], unet=build(cases.TINY_MOTION, torch.float32),
                                controlnet=build_controlnet(torch.float32)[0], scheduler=DDIMScheduler())
    kw = dict(video_length=F_TOT, height=128, width=128, latents=seeded_randn((1, 4, F_TOT, 16, 16), 5).to(DEV),
              text_embeddings=seeded_randn((2, 5, 32), 2), appearance_encoder=ref, ref_image_latents=seeded_randn((1, 4, 16, 16), 3), **LOOP_KW)
    path = str(tmp_path / "pose.gif")
    V.write_gif(torch.from_numpy(gif_ref.synthetic_clip(5, 128, 128, 9)).to(DEV), path, 25)
    with open(path, "rb") as f:
        frames = R.pillow_frames(f.read())                                       # what the file holds: the quantised frames
    from_frames = pipe("", controlnet_condition=frames[:F_TOT], **kw).videos
    assert torch.equal(pipe._clip_frames(path, F_TOT, 128, 128, "controlnet_condition").cpu(), torch.from_numpy(frames[:F_TOT]))
    assert torch.equal(pipe("", controlnet_condition=path, **kw).videos, from_frames)
    other = pipe("", controlnet_condition=frames[1:F_TOT + 1], **kw).videos
    assert not torch.equal(other, from_frames)                                   # and the frames matter
