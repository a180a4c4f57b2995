"""emo_image_resize (csrc/image_resize.hip) and what stands on it - video_io.resize_frames, read_video(size=), load_control_clip,
comparison_videos and the pipeline's input_resample= - against Pillow itself: `Image.fromarray(f).resize((w, h), filter)`.  Pillow's
resize of 8-bit images is integer arithmetic, so every comparison is an equality.  The kernel writes into poisoned buffers whose guard
must come back intact."""
import numpy as np
import pytest
import torch

from emote_hack_amd import video_io as V
from emote_hack_amd.synth import seeded_randn
from tests import image_resize_ref as R
from tests.test_gpu_jpeg_decode import F_TOT, intact, poisoned
from tests.test_gpu_kernels import DEV, ops

pytestmark = pytest.mark.gpu

# The horizontal pass gives a lane one pixel and a workgroup 256 of them; the vertical pass gives a lane one dword of the flat output
# (a workgroup 1024 bytes) and goes by whole dwords where rows are a multiple of 4 bytes (w % 4 == 0: 64, 40, 16, 8 of the shapes
# above), byte by byte where not (31, 129, 85 ...).  65 x 129 from 200 x 70: rows of 387 bytes, so dwords straddle rows and frames,
# and many workgroups in both passes.  4 x 100 -> 4 x 85 and 4 x 86: one frame is 340 and 344 pixels, 1020 and 1032 bytes, around
# what one workgroup writes.  -> 3 x 87: rows of 261 bytes through both passes.  -> 3 x 256 and 3 x 257: one workgroup's pixels a row.
STRADDLES = [((200, 70), (65, 129)), ((4, 100), (4, 85)), ((4, 100), (4, 86)), ((4, 100), (3, 87)), ((4, 100), (3, 256)), ((4, 100), (3, 257))]
SINGLE_AXIS = [((19, 128), (19, 31)), ((50, 7), (8, 7)), ((16, 16), (16, 16))]      # horizontal alone, vertical alone, neither


def device_taps(size_in, size_out, name):
    return None if size_in == size_out else tuple(torch.from_numpy(t.copy()).to(DEV) for t in V.resize_taps(size_in, size_out, name))


def device_resize(frames, h, w, name, xtaps=None, ytaps=None):
    """ops.image_resize of host frames into a poisoned buffer -> the host result"""
    n, H, W, _ = frames.shape
    buf, out = poisoned((n, h, w, 3), torch.uint8)
    got = ops().image_resize(torch.from_numpy(frames).to(DEV), h, w, xtaps or device_taps(W, w, name), ytaps or device_taps(H, h, name), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and intact((buf, out))
    return out.cpu().numpy()


def pillow(frames, h, w, name):
    return np.stack([R.pillow_resize(f, h, w, name) for f in frames])


@pytest.mark.parametrize("name", R.FILTERS)
@pytest.mark.parametrize("n", [1, 3])
def test_kernel_equals_pillow(name, n):
    for shape_in, shape_out in R.SHAPES + STRADDLES:
        frames = R.make_frames("noise", n, *shape_in, seed=n)
        assert np.array_equal(device_resize(frames, *shape_out, name), pillow(frames, *shape_out, name)), (shape_in, shape_out)


@pytest.mark.parametrize("content", ["checker", "white", "black"])
def test_overshoot_and_rounding(content):
    for name in R.FILTERS:
        for shape_in, shape_out in [((37, 53), (64, 64)), ((64, 64), (24, 40)), ((33, 21), (70, 50))]:
            frames = R.make_frames(content, 2, *shape_in)
            got = device_resize(frames, *shape_out, name)
            assert np.array_equal(got, pillow(frames, *shape_out, name)), (name, shape_in, shape_out)
            if content in ("white", "black"):
                assert (got == frames[0, 0, 0, 0]).all()
    if content == "checker":        # the case has what it is there for: an enlargement by bicubic reaches both ends of the range
        up = device_resize(R.make_frames("checker", 1, 33, 21), 70, 50, "bicubic")
        assert up.min() == 0 and up.max() == 255


def test_many_taps_and_a_one_pixel_axis():
    frames = R.make_frames("noise", 2, 300, 40)                                  # 60 : 1 by lanczos: 361 taps a row
    assert V.resize_taps(300, 5, "lanczos")[1].shape[1] == 361
    assert np.array_equal(device_resize(frames, 5, 40, "lanczos"), pillow(frames, 5, 40, "lanczos"))
    frames = R.make_frames("noise", 2, 1, 9)
    for name in R.FILTERS:
        assert np.array_equal(device_resize(frames, 16, 9, name), pillow(frames, 16, 9, name)), name


@pytest.mark.parametrize("shape_in,shape_out", SINGLE_AXIS)
def test_each_pass_alone_and_the_copy(shape_in, shape_out):
    frames = R.make_frames("noise", 3, *shape_in)
    lib, o = ops()._lib.load(), ops()
    assert lib.emo_image_resize_workspace_bytes(3, *shape_in, *shape_out) == 0               # one pass or none: no intermediate image
    for name in ("bicubic", "lanczos"):
        assert np.array_equal(device_resize(frames, *shape_out, name), pillow(frames, *shape_out, name)), name
    if shape_in == shape_out:                                                                # and no table is asked for
        assert np.array_equal(o.image_resize(torch.from_numpy(frames).to(DEV), *shape_out).cpu().numpy(), frames)


def test_vertical_pass_from_frames_that_are_not_dword_aligned():
    frames = R.make_frames("noise", 2, 21, 8)                                                # rows of 24 bytes, the frames one byte off
    flat = torch.zeros(frames.size + 4, device=DEV, dtype=torch.uint8)
    off = flat[1:1 + frames.size].view(frames.shape)
    off.copy_(torch.from_numpy(frames))
    assert off.data_ptr() % 4 == 1
    got = ops().image_resize(off, 9, 8, None, device_taps(21, 9, "bicubic"))
    assert np.array_equal(got.cpu().numpy(), pillow(frames, 9, 8, "bicubic"))


def test_resize_frames_surface():
    frames = R.make_frames("noise", 3, 37, 53)
    want = pillow(frames, 64, 48, "bicubic")
    got = V.resize_frames(torch.from_numpy(frames).to(DEV), (48, 64))
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(V.resize_frames(frames, (48, 64)).cpu().numpy(), want)              # a host array is uploaded
    one = V.resize_frames(frames[1], size=(48, 64), resample="Lanczos")                       # one frame keeps its rank
    assert one.is_cuda and np.array_equal(one.cpu().numpy(), R.pillow_resize(frames[1], 64, 48, "lanczos"))
    strided = torch.from_numpy(frames).to(DEV)[:, ::2, 1::2]                                   # a view is packed first
    assert np.array_equal(V.resize_frames(strided, (20, 10), "box").cpu().numpy(), pillow(np.ascontiguousarray(frames[:, ::2, 1::2]), 10, 20, "box"))


# ------------------------------------------------------------------------------------------------------------------- the C entry
def raw_call(o, frames, out, n, H, W, h, w, xt, yt, ws, ws_bytes):
    p = o._ptr
    return o._lib.load().emo_image_resize(p(frames), p(out), n, H, W, h, w, p(xt and xt[0]), p(xt and xt[1]), xt[1].shape[1] if xt else 0,
                                          p(yt and yt[0]), p(yt and yt[1]), yt[1].shape[1] if yt else 0, p(ws), ws_bytes, o._stream())


def test_entry_point_refusals():
    o = ops()
    lib = o._lib.load()
    n, H, W, h, w = 2, 20, 30, 10, 12
    frames = torch.from_numpy(R.make_frames("noise", n, H, W)).to(DEV)
    xt, yt = device_taps(W, w, "bicubic"), device_taps(H, h, "bicubic")
    need = lib.emo_image_resize_workspace_bytes(n, H, W, h, w)
    assert need == n * H * w * 3
    wbuf, ws = poisoned((need,), torch.uint8)
    buf, out = poisoned((n, h, w, 3), torch.uint8)
    BAD_SHAPE, NULL = -1, -5
    assert raw_call(o, frames, out, n, H, W, h, w, xt, yt, ws, need - 1) == BAD_SHAPE        # a workspace one byte short
    assert b"workspace" in lib.emo_last_error_string()
    assert raw_call(o, frames, out, n, H, W, h, w, xt, yt, None, need) == NULL
    assert raw_call(o, None, out, n, H, W, h, w, xt, yt, ws, need) == NULL
    assert raw_call(o, frames, None, n, H, W, h, w, xt, yt, ws, need) == NULL
    assert raw_call(o, frames, out, n, H, W, h, w, None, yt, ws, need) == NULL               # the width changes: its tables are needed
    assert raw_call(o, frames, out, n, H, W, h, w, xt, None, ws, need) == NULL
    for bad in ((0, H, W, h, w), (n, 0, W, h, w), (n, H, W, h, 0), (n, H, W, -3, w), (1, 30000, 30000, h, w), (1, H, W, 30000, 30000),
                (1, 60000, 8, 8, 60000)):                                                    # the last: only the intermediate image is too large
        assert raw_call(o, frames, out, *bad, xt, yt, ws, need) == BAD_SHAPE, bad
        assert lib.emo_image_resize_workspace_bytes(*bad) == 0
    assert raw_call(o, frames, frames, n, H, W, h, w, xt, yt, ws, need) == BAD_SHAPE         # in place
    torch.cuda.synchronize()
    assert intact((buf, out), (wbuf, ws)) and bool((out == 0xA5).all()) and bool((ws == 0xA5).all())      # nothing was launched
    assert raw_call(o, frames, out, n, H, W, h, w, xt, yt, ws, need) == 0                    # and the same call with what it needs
    torch.cuda.synchronize()
    assert intact((buf, out), (wbuf, ws))
    host = frames.cpu().numpy()
    assert np.array_equal(out.cpu().numpy(), pillow(host, h, w, "bicubic"))
    assert np.array_equal(ws.view(n, H, w, 3).cpu().numpy(), pillow(host, H, w, "bicubic"))   # the intermediate image is Pillow's too


@pytest.mark.parametrize("w", [14, 16])                                         # rows of 42 bytes, and of 48: the vertical pass by dwords
def test_tables_that_point_outside_the_image_are_clamped(w):
    """a wrong answer, never a fault: `first` is clamped to the axis, `count` to the table's width and to what the axis has left"""
    n, H, W, h = 2, 12, 20, 9
    frames = R.make_frames("noise", n, H, W)
    tabs = {}
    for axis, (size_in, size_out) in (("x", (W, w)), ("y", (H, h))):
        bounds, coef = (t.copy() for t in V.resize_taps(size_in, size_out, "bicubic"))
        k = coef.shape[1]
        wild = [(-5, 3), (size_in - 1, k), (size_in + 7, 2), (2 ** 31 - 1, 2 ** 31 - 1), (-2 ** 31, k), (0, -4), (3, 10 * k), (size_in - 2, k)]
        bounds[:len(wild)] = wild
        coef[len(wild) - 1] = 2 ** 31 - 1                                        # and sums that wrap
        tabs[axis] = (bounds, coef)
    dev = {a: tuple(torch.from_numpy(t).to(DEV) for t in tabs[a]) for a in tabs}
    got = device_resize(frames, h, w, "bicubic", xtaps=dev["x"], ytaps=dev["y"])      # (asserts the guard)

    def clamped(bounds, coef, size_in):
        first = np.clip(bounds[:, 0].astype(np.int64), 0, size_in - 1)
        count = np.clip(bounds[:, 1].astype(np.int64), 0, np.minimum(coef.shape[1], size_in - first))
        return np.stack([first, count], axis=1)

    def wrapping_pass(x, axis, bounds, coef):                                    # resample_axis with 32-bit wrap-around
        x = np.moveaxis(x, axis, 0).astype(np.int64)
        out = np.empty((len(bounds),) + x.shape[1:], np.uint8)
        for o_, (first, count) in enumerate(bounds):
            acc = np.tensordot(coef[o_, :count].astype(np.int64), x[first:first + count], axes=1) + (1 << 21)
            acc = ((acc + 2 ** 31) % 2 ** 32) - 2 ** 31
            out[o_] = np.clip(acc >> 22, 0, 255)
        return np.moveaxis(out, 0, axis)

    mid = wrapping_pass(frames, 2, clamped(*tabs["x"], W), tabs["x"][1])
    want = wrapping_pass(mid, 1, clamped(*tabs["y"], H), tabs["y"][1])
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------------- clips
CLIP_H, CLIP_W = 96, 160


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """a 5-frame 96 x 160 clip -> (path, Pillow's decoding of its frames)"""
    from tests import jpeg_decode_ref as D
    from tests import mjpeg_ref as M
    path = str(tmp_path_factory.mktemp("resize") / "pose.avi")
    frames = torch.from_numpy(np.stack([D.picture(CLIP_H, CLIP_W, 30 + i) for i in range(F_TOT + 1)])).to(DEV)
    V.write_video(frames, path, 25, 90)
    return path, np.stack([M.decode(j) for j in V.read_avi(path)[0]])


def test_read_video_resizes(clip):
    path, decoded = clip
    got, fps, _ = V.read_video(path, size=(128, 128))
    assert got.is_cuda and fps == 25 and np.array_equal(got.cpu().numpy(), pillow(decoded, 128, 128, "bicubic"))
    got, _, _ = V.read_video(path, start=1, step=2, length=2, size=(40, 24), resample="hamming")
    assert np.array_equal(got.cpu().numpy(), pillow(decoded[1::2][:2], 24, 40, "hamming"))
    same, _, _ = V.read_video(path, size=(CLIP_W, CLIP_H))                      # at size already: the decoded frames
    assert np.array_equal(same.cpu().numpy(), decoded)


def test_load_control_clip(clip):
    path, decoded = clip
    frames, original_length = V.load_control_clip(path, (128, 128), 4)
    assert frames.is_cuda and frames.dtype == torch.uint8 and tuple(frames.shape) == (8, 128, 128, 3) and original_length == 5
    host = frames.cpu().numpy()
    assert np.array_equal(host[:5], pillow(decoded, 128, 128, "bicubic"))
    assert all(np.array_equal(host[i], host[4]) for i in (5, 6, 7))
    frames, original_length = V.load_control_clip(path, (64, 48), 2, offset=1, max_length=3, resample="bilinear")
    assert original_length == 3 and np.array_equal(frames.cpu().numpy(), pillow(decoded[[1, 2, 3, 3]], 48, 64, "bilinear"))


def test_comparison_videos(clip, tmp_path):
    path, decoded = clip
    control, original_length = V.load_control_clip(path, (32, 24), 4)
    source = decoded[0, :24, :32]
    sample = seeded_randn((1, 3, 8, 24, 32), 11).abs().clamp(0, 1).to(DEV)
    grid = V.comparison_videos(source, control, sample, original_length)
    assert grid.is_cuda and grid.dtype == torch.float32 and tuple(grid.shape) == (3, 3, 5, 24, 32)
    host = grid.cpu().numpy()
    want_source = np.broadcast_to((source / 255.0).astype(np.float32).transpose(2, 0, 1)[:, None], (3, 5, 24, 32))     # animation.py:217-218
    want_control = (control.cpu().numpy()[:5] / 255.0).astype(np.float32).transpose(3, 0, 1, 2)                          # :221-224
    assert np.array_equal(host[0], want_source) and np.array_equal(host[1], want_control)
    assert np.array_equal(host[2], sample.cpu().numpy()[0, :, :5])                                                       # :226
    assert torch.equal(V.comparison_videos(torch.from_numpy(np.ascontiguousarray(source)).to(DEV), control, sample, 5), grid)
    out = str(tmp_path / "grid.avi")
    V.save_videos_grid(grid, out)                                                # :233
    jpegs, fps, _ = V.read_avi(out)
    assert len(jpegs) == 5 and fps == 25
    p = V.parse_jpeg(jpegs[0])
    assert (p.height, p.width) == (24 + 4, 3 * (32 + 2) + 2)                     # make_grid: three cells in a row
    for bad in (0, 6, 9):
        with pytest.raises(ValueError, match="original_length"):
            V.comparison_videos(source, control[:5], sample, bad)
    with pytest.raises(ValueError, match="source_u8"):
        V.comparison_videos(decoded[0], control, sample, 5)


# ------------------------------------------------------------------------------------------------------------------- pipeline
def test_pipeline_resizes_clips_under_input_resample(clip):
    path, decoded = clip
    e = _tiny_env()
    pipe, kw = e["pipe"], e["kw"]
    ref_lat = seeded_randn((1, 4, 16, 16), 3)
    by_pillow = pillow(decoded[:F_TOT], 128, 128, None)                          # Image.fromarray(f).resize((128, 128)), no filter named
    from_clip = pipe("", controlnet_condition=path, ref_image_latents=ref_lat, input_resample="bicubic", **kw).videos
    from_frames = pipe("", controlnet_condition=by_pillow, ref_image_latents=ref_lat, **kw).videos
    assert torch.equal(from_clip, from_frames)
    other = pipe("", controlnet_condition=path, ref_image_latents=ref_lat, input_resample="lanczos", **kw).videos
    assert not torch.equal(other, from_clip)                                     # the filter matters
    src_clip = pipe("", controlnet_condition=by_pillow, source_image=path, input_resample="bicubic", **kw).videos
    src_frame = pipe("", controlnet_condition=by_pillow, source_image=by_pillow[0], **kw).videos
    assert torch.equal(src_clip, src_frame) and not torch.equal(src_clip, from_frames)
    # opt-in: without it the clip is refused as before; a clip that is too short is refused with it; an unknown filter by name
    with pytest.raises(ValueError, match="pass frames at size"):
        pipe("", controlnet_condition=path, ref_image_latents=ref_lat, **kw)
    long = dict(kw, video_length=8, latents=seeded_randn((1, 4, 8, 16, 16), 5).to(DEV))
    with pytest.raises(ValueError, match="holds 5 frames, 8 are needed"):
        pipe("", controlnet_condition=path, ref_image_latents=ref_lat, input_resample="bicubic", **long)
    with pytest.raises(ValueError, match="nearest-neighbour resizing is not built"):
        pipe("", controlnet_condition=path, ref_image_latents=ref_lat, input_resample="nearest", **kw)


def _tiny_env():
    """the tiny pipeline of tests/test_gpu_jpeg_decode.py's clip tests, built from the same helpers"""
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    from tests import cases
    from tests.test_gpu_controlnet import build_controlnet
    from tests.test_gpu_jpeg_decode import LOOP_KW
    from tests.test_gpu_unet import build
    from tests.test_gpu_vae import SMALL, build as build_vae
    ref = build(cases.TINY, torch.float32, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    pipe = EMOAnimationPipeline(vae=build_vae(SMALL, torch.float32)[0], unet=build(cases.TINY_MOTION, torch.float32),
                                controlnet=build_controlnet(torch.float32)[0], scheduler=DDIMScheduler())
    kw = dict(video_length=F_TOT, height=128, width=128, latents=seeded_randn((1, 4, F_TOT, 16, 16), 5).to(DEV),
              text_embeddings=seeded_randn((2, 5, 32), 2), appearance_encoder=ref, **LOOP_KW)
    return dict(pipe=pipe, kw=kw)
