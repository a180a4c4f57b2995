"""GPU tests of the PNG / APNG reader: emo_png_inflate and emo_png_unfilter (csrc/png_in.hip) against zlib, a numpy restatement and
Pillow, and decode_png / decode_apng / read_image / read_video on files of this project's writer and of Pillow.  Every comparison is
byte for byte.  The streams are those of tests/png_decode_cases.py, whose claims (block types, match lengths and distances, the ring's
wrap, 15-bit codes, ...) tests/test_png_decode_host.py asserts from the serial reference's record.

The outputs of the two entries lie inside larger buffers filled with a guard byte, which every test checks: a damaged stream gives a
status, and nothing outside the frame's own bytes is written."""
import functools
import io
import zlib
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
from tests import png_decode_cases as K
from tests import png_decode_ref as D
from tests import png_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, POISON = 256, 0xA5


def guarded(shape):
    """a uint8 tensor of `shape` inside a buffer of guard bytes -> (the tensor, a check of the guards)"""
    size = int(np.prod(shape))
    whole = torch.full((size + 2 * GUARD,), POISON, dtype=torch.uint8, device=DEV)

    def intact():
        host = whole.cpu().numpy()
        return bool((host[:GUARD] == POISON).all() and (host[GUARD + size:] == POISON).all())
    return whole[GUARD:GUARD + size].view(*shape), intact


def upload(streams):
    sizes = np.array([len(s) for s in streams], np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pad = -int(offsets[-1]) % 4 or (4 if offsets[-1] == 0 else 0)
    data = np.frombuffer(b"".join(streams) + bytes([POISON]) * pad, np.uint8)     # what lies behind the last frame is not zeros
    return torch.from_numpy(data.copy()).to(DEV), torch.from_numpy(offsets).to(DEV)


def inflate(streams, nbytes):
    """-> (filtered as bytes per frame, produced, status); the guards around filtered are checked"""
    H, W, C = K.shape_of(nbytes)
    out, intact = guarded((len(streams), H, 1 + W * C))
    filtered, produced, status = ops.png_inflate(*upload(streams), H, W, C, out=out)
    torch.cuda.synchronize()
    assert intact(), "emo_png_inflate wrote outside filtered"
    host = filtered.cpu().numpy().reshape(len(streams), -1)
    return [h.tobytes() for h in host], produced.cpu().numpy().tolist(), status.cpu().numpy().tolist()


# ------------------------------------------------------------------------------------------------------------------------------ inflate
@pytest.mark.parametrize("name", sorted(K.all_streams()))
def test_inflate_equals_zlib(name):
    stream, _ = K.all_streams()[name]
    want = K.raw_inflate(stream)
    got, produced, status = inflate([stream], len(want))
    assert status == [D.OK] and produced == [len(want)]
    assert got[0] == want


def test_frames_of_different_stream_lengths_share_a_launch():
    s = K.all_streams()
    for names in (("pillow_noise64", "pillow_flat", "pillow_gradient", "pillow_flat", "pillow_noise64"), ("far_source", "far_dest", "far_source")):
        streams = [s[k][0] for k in names]
        assert len({len(x) for x in streams}) > 1 and len({len(s[k][1]) for k in names}) == 1
        got, produced, status = inflate(streams, len(s[names[0]][1]))
        assert status == [D.OK] * len(names) and produced == [len(s[names[0]][1])] * len(names)
        for k, g in zip(names, got):
            assert g == K.raw_inflate(s[k][0]), k


@pytest.mark.parametrize("name", sorted(K.damaged_streams()))
def test_a_damaged_stream_gives_its_status_and_touches_nothing_else(name):
    stream, want = K.damaged_streams()[name]
    if want not in (D.OVERFLOW, D.SHORT):
        with pytest.raises(zlib.error):
            K.raw_inflate(stream)
    good, data = K.healthy()
    got, produced, status = inflate([good, stream, good], K.SMALL)
    ref_bytes, ref_status, _ = D.inflate(stream, K.SMALL)
    assert ref_status == want
    assert status == [D.OK, want, D.OK], (name, status)
    assert got[0] == data and got[2] == data and produced[0] == produced[2] == K.SMALL
    assert produced[1] == len(ref_bytes) <= K.SMALL and got[1][:produced[1]] == ref_bytes


def test_offsets_that_run_backwards_or_leave_the_buffer_are_an_empty_frame():
    good, data = K.healthy()
    streams, offsets = upload([good, good])
    n = len(good)
    for bad, want in (([0, n, n - 5], [D.OK, D.PAST_END]), ([0, n, 2 * n + 64], [D.OK, D.PAST_END]), ([-8, n, 2 * n], [D.PAST_END, D.OK])):
        out, intact = guarded((2, 1, K.SMALL))
        off = torch.tensor(bad, dtype=torch.int64, device=DEV)
        filtered, produced, status = ops.png_inflate(streams, off, *K.shape_of(K.SMALL), out=out)
        torch.cuda.synchronize()
        assert intact()
        assert status.cpu().numpy().tolist() == want, bad
        healthy = want.index(D.OK)
        assert filtered[healthy].cpu().numpy().tobytes() == data and int(produced[1 - healthy]) == 0


def test_entries_refuse_bad_shapes_before_any_launch():
    streams, offsets = upload([K.healthy()[0]])
    for H, W, C in ((1, 99, 5), (1, 99, 0), (0, 99, 1), (1, 0, 1), (65536, 32767, 1)):
        with pytest.raises(EmoHipError, match="emo_png_inflate"):
            ops._lib.check(ops._lib.load().emo_png_inflate(ops._ptr(streams), streams.numel(), ops._ptr(offsets), ops._ptr(streams), ops._ptr(offsets),
                                                           ops._ptr(offsets), 1, H, W, C, None), "emo_png_inflate")
        with pytest.raises(EmoHipError, match="emo_png_unfilter"):
            ops._lib.check(ops._lib.load().emo_png_unfilter(ops._ptr(streams), ops._ptr(streams), ops._ptr(offsets), ops._ptr(offsets), 1, H, W, C, None),
                           "emo_png_unfilter")
    with pytest.raises(EmoHipError, match="multiple of 4"):
        ops._lib.check(ops._lib.load().emo_png_inflate(ops._ptr(streams), streams.numel() - 1, ops._ptr(offsets), ops._ptr(streams), ops._ptr(offsets),
                                                       ops._ptr(offsets), 1, 1, 99, 1, None), "emo_png_inflate")
    with pytest.raises(EmoHipError, match="98304"):
        ops._lib.check(ops._lib.load().emo_png_unfilter(ops._ptr(streams), ops._ptr(streams), ops._ptr(offsets), ops._ptr(offsets), 1, 1, 24577, 4, None),
                       "emo_png_unfilter")


# ------------------------------------------------------------------------------------------------------------------------------ unfilter
HEIGHTS, WIDTHS = (1, 2, 63, 64, 65, 130), (1, 2, 5, 64, 67)


@functools.lru_cache(maxsize=None)
def picture(H, W, C):
    """(2, H, W, C): smooth ramps with noise on them, so that the adaptive choice mixes the types; the second frame's row 0 has zeros
    above it, not the first frame's last row"""
    rng = np.random.default_rng(1000 * H + 10 * W + C)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([3 * x + 5 * y, 7 * x - 2 * y + 40, 200 - x * y // 3, 255 - 4 * x][:C], axis=-1)[None] + np.array([0, 90]).reshape(2, 1, 1, 1)
    noise = rng.integers(-2, 3, (2, H, W, C)) * (rng.integers(0, 4, (2, H, 1, 1)) > 0)      # some rows without any
    frames = ((base + noise) % 256).astype(np.uint8)
    for r in range(H):                                                           # rows that None, Up and Sub win, between the ramps
        if r % 5 == 0:
            frames[:, r] = np.where(np.arange(W) % 2 == 0, 1, 255).astype(np.uint8).reshape(1, W, 1)
        elif r % 5 == 2:
            frames[:, r] = frames[:, r - 1] + rng.integers(0, 2, (2, W, C), dtype=np.uint8)
        elif r % 5 == 4:
            frames[:, r] = (7 * np.arange(W) + r).astype(np.uint8).reshape(1, W, 1)
    frames.setflags(write=False)
    return frames


def unfilter(filtered, C):
    """-> (frames, adler, status) as numpy; the guards around frames are checked"""
    n, H, R = filtered.shape
    out, intact = guarded((n, H, (R - 1) // C, C))
    frames, adler, status = ops.png_unfilter(torch.from_numpy(np.ascontiguousarray(filtered)).to(DEV), C, out=out)
    torch.cuda.synchronize()
    assert intact(), "emo_png_unfilter wrote outside frames"
    return frames.cpu().numpy(), adler.cpu().numpy(), status.cpu().numpy().tolist()


@pytest.mark.parametrize("filter", range(6))
@pytest.mark.parametrize("C", (1, 2, 3, 4))
def test_unfilter_undoes_every_filter_type_on_every_row(C, filter):
    for H in HEIGHTS:
        for W in WIDTHS:
            frames = picture(H, W, C)
            filtered = png_ref.filter_frames(frames, filter)                     # the type forced on every row, the first of a frame and of a band too
            got, adler, status = unfilter(filtered, C)
            assert status == [D.OK, D.OK], (H, W)
            assert np.array_equal(got, frames), (H, W)
            assert np.array_equal(adler.astype(np.int64), png_ref.adler_pairs(filtered)), (H, W)
            if filter == 5 and H == 130 and W >= 64:
                assert all(len(set(filtered[f, band:band + 64, 0].tolist())) >= 3 for f in range(2) for band in (0, 64)), "types do not mix in a band"


def test_unfilter_equals_the_numpy_restatement_on_independent_bytes():
    rng = np.random.default_rng(77)
    for C in (1, 2, 3, 4):
        filtered = rng.integers(0, 256, (2, 70, 1 + 66 * C), dtype=np.uint8)      # no picture behind them: every predictor wraps
        filtered[:, :, 0] = rng.integers(0, 5, (2, 70))
        got, adler, status = unfilter(filtered, C)
        assert status == [D.OK, D.OK] and np.array_equal(got, D.unfilter(filtered, C))
        assert np.array_equal(adler.astype(np.int64), png_ref.adler_pairs(filtered))


def test_a_filter_type_above_4_gives_its_status_and_touches_nothing_else():
    frames = picture(65, 67, 3)
    filtered = np.concatenate([png_ref.filter_frames(frames, 4)] * 2)[:3].copy()
    filtered[1, 64, 0] = 5                                                       # in the second band of the middle frame
    got, adler, status = unfilter(filtered, 3)
    assert status == [D.OK, D.BAD_FILTER, D.OK]
    assert np.array_equal(got[0], frames[0]) and np.array_equal(got[2], frames[0])
    assert np.array_equal(got[1, :64], frames[1, :64]) and (got[1, 64] == POISON).all()
    with pytest.raises(ValueError):
        D.unfilter(filtered, 3)


# ------------------------------------------------------------------------------------------------------------------------------ files
@functools.lru_cache(maxsize=None)
def clip(C):
    frames = picture(37, 53, 3)
    frames = {1: frames[..., 1:2], 3: frames, 4: np.concatenate([frames, 255 - frames[..., :1]], axis=3)}[C]
    return frames.copy()


@pytest.mark.parametrize("filter", sorted(ops.PNG_FILTERS))
def test_what_the_writer_writes_reads_back(filter):
    for C in (1, 3, 4):
        x = torch.from_numpy(clip(C)).to(DEV)
        for strip_rows in (1, 8):
            files = V.encode_png(x, filter=filter, strip_rows=strip_rows)
            got = V.decode_png(files)
            assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got, x), (C, strip_rows)
            frames, delays, loop = V.decode_apng(V.encode_apng(x, Fraction(30000, 1001), loop=3, filter=filter, strip_rows=strip_rows))
            assert torch.equal(frames, x) and delays == [Fraction(1001, 30000)] * 2 and loop == 3


@functools.lru_cache(maxsize=None)
def pillow_stills():
    """mode -> (the file, its array): sizes past one band and one chunk, Pillow's own choice of filters and blocks"""
    out = {}
    for mode, C in (("L", 1), ("LA", 2), ("RGB", 3), ("RGBA", 4)):
        a = picture(70, 90, C)[0]
        a = a[..., 0] if C == 1 else a
        out[mode] = (K.pillow_file(a), a)
    return out


@pytest.mark.parametrize("mode", ("L", "LA", "RGB", "RGBA"))
def test_pillow_files_decode_as_pillow_decodes_them(mode, tmp_path):
    data, a = pillow_stills()[mode]
    im = Image.open(io.BytesIO(data))
    assert im.mode == mode
    got = V.decode_png([data, data])
    assert np.array_equal(got[1].cpu().numpy().reshape(a.shape), np.asarray(im))
    rgb = np.asarray(im.convert("RGB"))
    path = tmp_path / "still.png"
    path.write_bytes(data)
    for src in (data, str(path), path):
        got = V.read_image(src)
        assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), rgb)
    for size, resample, pil in (((64, 48), "bicubic", Image.BICUBIC), ((40, 24), "bilinear", Image.BILINEAR)):
        want = np.array(Image.open(io.BytesIO(data)).convert("RGB").resize(size, pil))
        assert np.array_equal(V.read_image(data, size=size, resample=resample).cpu().numpy(), want), size


def test_pillow_files_with_stored_fixed_and_dynamic_blocks():
    for name, a in K.pillow_images().items():
        got = V.decode_png([K.pillow_files()[name]])
        assert np.array_equal(got[0].cpu().numpy(), a), name


def test_decode_png_names_the_frame_it_refuses():
    good = pillow_stills()["RGB"][0]
    p = V.parse_png(good)
    filtered = bytearray(K.raw_inflate(p.still))
    wrong_adler = V.png_container(p.width, p.height, 3, b"\x78\x01" + p.still + (p.still_adler ^ 1).to_bytes(4, "big"))
    filtered[5 * (1 + 3 * p.width)] = 5
    filter5 = V.png_container(p.width, p.height, 3, zlib.compress(bytes(filtered)))
    cut = V.png_container(p.width, p.height, 3, b"\x78\x01" + p.still[:len(p.still) // 2] + p.still_adler.to_bytes(4, "big"))
    crc = bytearray(good)
    crc[60] ^= 4
    for bad, words in ((wrong_adler, "Adler-32"), (filter5, "filter type above 4"), (cut, "emo_png_inflate status"), (bytes(crc), "CRC mismatch")):
        with pytest.raises(OSError):
            Image.open(io.BytesIO(bad)).load()
        with pytest.raises(ValueError, match="frame 1") as e:
            V.decode_png([good, bad, good])
        assert words in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="frame 1 is 70 x 90 x 4"):              # a sound file of another colour type
        V.decode_png([good, pillow_stills()["RGBA"][0], good])
    with pytest.raises(ValueError, match="read_image: .*palette"):
        buf = io.BytesIO()
        Image.fromarray(picture(8, 8, 3)[0]).convert("P").save(buf, "PNG")
        V.read_image(buf.getvalue())


def test_read_video(tmp_path):
    x = torch.from_numpy(np.ascontiguousarray(picture(40, 56, 3)[[0, 1, 0, 1, 1, 0, 0]] + np.arange(7, dtype=np.uint8).reshape(7, 1, 1, 1))).to(DEV)
    V.write_video(x, str(tmp_path / "clip.apng"), 25, format="apng")
    (tmp_path / "anim.png").write_bytes((tmp_path / "clip.apng").read_bytes())
    paths = V.write_png(x, str(tmp_path / "f_%04d.png"))
    for k, p in enumerate(V.write_png(x, str(tmp_path / "from_one" / "g_%d.png"))):           # a sequence counted from 1
        (tmp_path / "from_one" / f"h_{k + 1}.png").write_bytes(open(p, "rb").read())
    for path, fps in (("clip.apng", 25), ("anim.png", 25), ("f_%04d.png", None), ("from_one/h_%d.png", None)):
        got, rate, audio = V.read_video(tmp_path / path)
        assert got.is_cuda and torch.equal(got, x) and rate == fps and audio is None, path
        for kw in (dict(step=2, length=2, start=1), dict(step=4, length=16, start=0), dict(step=1, length=3, start=5)):
            part, _, _ = V.read_video(str(tmp_path / path), **kw)
            assert torch.equal(part, x[kw["start"]::kw["step"]][:kw["length"]]), (path, kw)
            assert np.array_equal(np.stack(V.video2images(str(tmp_path / path), **kw)), part.cpu().numpy())
        with pytest.raises(ValueError, match="selects none"):
            V.read_video(tmp_path / path, start=7)
        small, _, _ = V.read_video(tmp_path / path, size=(28, 20), length=2)
        assert torch.equal(small, V.resize_frames(x[:2], (28, 20)))
    frames, original = V.load_control_clip(tmp_path / "f_%04d.png", (56, 40), 4)
    assert original == 7 and tuple(frames.shape) == (8, 40, 56, 3) and torch.equal(frames[:7], x) and torch.equal(frames[7], x[6])
    # a file of Pillow's with whole frames, delays that differ, grey + alpha
    la = [Image.fromarray(K.noise((20, 30, 2), 30 + i), "LA") for i in range(3)]
    la[0].save(tmp_path / "pillow.apng", format="PNG", save_all=True, append_images=la[1:], duration=[40, 40, 100], loop=0)
    got, rate, _ = V.read_video(tmp_path / "pillow.apng")
    with Image.open(tmp_path / "pillow.apng") as im:
        assert im.n_frames == 3
        want = []
        for i in range(3):
            im.seek(i)
            want.append(np.asarray(im.convert("RGB")))
    assert rate is None and np.array_equal(got.cpu().numpy(), np.stack(want))
    frames, delays, loop = V.decode_apng((tmp_path / "pillow.apng").read_bytes())
    assert delays == [Fraction(1, 25), Fraction(1, 25), Fraction(1, 10)] and loop == 0 and tuple(frames.shape) == (3, 20, 30, 2)


# ------------------------------------------------------------------------------------------------------------------------------ pipeline
F_TOT = 4
LOOP_KW = dict(num_inference_steps=2, guidance_scale=7.5, context_frames=4, context_stride=1, context_overlap=0, seed=0, output_type="latent")


def test_control_frames_from_numbered_stills_reach_the_loop(tmp_path):
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
    frames = np.ascontiguousarray(picture(128, 128, 3)[[0, 1, 1, 0, 0]] + np.arange(5, dtype=np.uint8).reshape(5, 1, 1, 1) * 9)
    (tmp_path / "pose").mkdir()
    V.write_png(torch.from_numpy(frames).to(DEV), str(tmp_path / "pose" / "%04d.png"))
    V.write_video(torch.from_numpy(frames).to(DEV), str(tmp_path / "pose.apng"), 25, format="apng")
    from_frames = pipe("", controlnet_condition=frames[:F_TOT], **kw).videos
    for path in (str(tmp_path / "pose" / "%04d.png"), str(tmp_path / "pose.apng")):
        assert torch.equal(pipe._clip_frames(path, F_TOT, 128, 128, "controlnet_condition").cpu(), torch.from_numpy(frames[:F_TOT]))
        assert torch.equal(pipe("", controlnet_condition=path, **kw).videos, from_frames), path
    other = pipe("", controlnet_condition=frames[1:F_TOT + 1], **kw).videos
    assert not torch.equal(other, from_frames)                                   # and the frames matter


def test_a_png_portrait_read_on_the_device_gives_the_latents_of_its_pixels(tmp_path):
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    from tests.test_gpu_unet import build
    from tests.test_gpu_vae import SMALL, build as build_vae
    pipe = EMOAnimationPipeline(vae=build_vae(SMALL, torch.float32)[0], unet=build(cases.TINY_MOTION, torch.float32), scheduler=DDIMScheduler())
    path = str(tmp_path / "portrait.png")
    Image.fromarray(picture(96, 120, 4)[0], "RGBA").save(path)
    on_device = V.read_image(path, size=(64, 64))
    want = np.array(Image.open(path).convert("RGB").resize((64, 64)))
    assert on_device.is_cuda and np.array_equal(on_device.cpu().numpy(), want)
    from_path = pipe._source_image_latents(path, 64, 64)
    from_device = pipe._source_image_latents(on_device, 64, 64)
    assert tuple(from_path.shape) == (1, 4, 8, 8) and float(from_path.abs().max()) > 0
    assert torch.allclose(from_path.to(DEV), from_device.to(DEV), rtol=1e-3, atol=1e-4)
