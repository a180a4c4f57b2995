"""GPU tests of the JPEG layouts: emo_jpeg_decode_bits / _decode_segments / _idct / _rgb (csrc/video_in.hip) in every layout through
their ops wrappers against the numpy restatement in tests/jpeg_layout_ref.py (which tests/test_jpeg_layouts_host.py holds to Pillow's decoder
byte for byte), decode_mjpeg and read_image against Pillow's decoder itself - 4:4:4, 4:2:2, 4:2:0 and grey files, with and without
restart intervals, mixed in one call - and the pipeline taking its source image from a still JPEG file on the device.

Everything but the VAE is integer arithmetic, so every comparison is an equality.  Every output a kernel writes is the front of a larger
buffer whose tail holds a poison value that must come back untouched."""
import functools
import io

import numpy as np
import pytest
import torch

from emote_hack_amd import video_io as V
from tests import jpeg_decode_ref as D
from tests import jpeg_layout_ref as L
from tests.test_gpu_jpeg_decode import device_decode_tables, intact, poisoned
from tests.test_gpu_kernels import DEV, ops

pytestmark = pytest.mark.gpu
CASES = [(name, H, W) for name in L.LAYOUTS for H, W in L.SIZES[name]]
RESTARTS = [dict(), dict(restart_marker_blocks=1), dict(restart_marker_blocks=2), dict(restart_marker_rows=1)]


@functools.lru_cache(maxsize=None)
def case(name, H, W, quality, optimize, restart=()):
    """(the file, every stage of the restatement of it): made once, shared, never written to"""
    data = L.pillow_file(D.picture(H, W, H * W + quality), name, quality, optimize, **dict(restart))
    return data, L.decode_all(data)


def to_dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).to(DEV)


def packed_scans(parts):
    """(the segments back to back on the device, padded to whole dwords; their int64 offsets)"""
    sizes = np.array([len(p) for p in parts], np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    scan = np.concatenate(list(parts) + [np.zeros(-int(offsets[-1]) % 4 or (0 if offsets[-1] else 4), np.uint8)])
    return to_dev(scan), offsets


def decode_bits(o, parts, specs, n_mcu, layout):
    """ops.jpeg_decode_bits on one whole scan per frame, into poisoned buffers -> (coefficients, status) on the host"""
    scan, offsets = packed_scans(parts)
    cb, coefs = poisoned((len(parts), n_mcu, L.bpm(layout), 64), torch.int16)
    sb, status = poisoned((len(parts),), torch.int32)
    o.jpeg_decode_bits(scan, to_dev(offsets), device_decode_tables(specs), n_mcu, layout=layout, out=coefs, status=status)
    torch.cuda.synchronize()
    assert intact((cb, coefs), (sb, status))
    return coefs.cpu().numpy(), status.cpu().numpy()


def decode_segments(o, frames, specs, n_mcu, layout):
    """ops.jpeg_decode_segments on frames = [(ri, parts)], into poisoned buffers -> (coefficients, status per segment)"""
    b, parts, first, blocks = L.bpm(layout), [], [], []
    for f, (ri, fparts) in enumerate(frames):
        spans = [(m0, min(m0 + (ri or n_mcu), n_mcu)) for m0 in range(0, n_mcu, ri or n_mcu)]
        assert len(spans) == len(fparts)
        parts += list(fparts)
        first += [(f * n_mcu + m0) * b for m0, _ in spans]
        blocks += [(m1 - m0) * b for m0, m1 in spans]
    scan, offsets = packed_scans(parts)
    cb, coefs = poisoned((len(frames), n_mcu, b, 64), torch.int16)
    sb, status = poisoned((len(parts),), torch.int32)
    o.jpeg_decode_segments(scan, to_dev(offsets), to_dev(first, np.int32), to_dev(blocks, np.int32), device_decode_tables(specs),
                           len(frames), n_mcu, layout=layout, out=coefs, status=status)
    torch.cuda.synchronize()
    assert intact((cb, coefs), (sb, status))
    return coefs.cpu().numpy(), status.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------- the four kernels
@pytest.mark.parametrize("name,H,W", CASES)
def test_kernels_equal_the_restatement(name, H, W):
    o, layout = ops(), L.LAYOUTS[name]
    mr, mc = L.grid(H, W, layout)
    n_mcu, (nc, hs, vs) = mr * mc, layout
    assert o.jpeg_grid(H, W, layout) == (mr, mc) and o.jpeg_bpm(layout) == L.bpm(layout)
    for quality in L.QUALITIES:
        for optimize in (False, True):
            _, (f, want, want_y, want_c, want_rgb) = case(name, H, W, quality, optimize)
            # both entropy entries: the frame as one workgroup's, and as one wavefront's segment
            got, status = decode_bits(o, f["parts"], f["specs"], n_mcu, layout)
            assert not status.any() and np.array_equal(got[0], want), (quality, optimize, status)
            got, status = decode_segments(o, [(0, f["parts"])], f["specs"], n_mcu, layout)
            assert not status.any() and np.array_equal(got[0], want), (quality, optimize, status)
            # the planes
            yb, y = poisoned((1, mr * 8 * vs, mc * 8 * hs), torch.uint8)
            cb, c = poisoned((1, 2, mr * 8, mc * 8), torch.uint8) if nc == 3 else (None, None)
            o.jpeg_idct(to_dev(want[None]), to_dev(f["quant"], np.uint16), H, W, layout=layout, out_y=y, out_c=c)
            assert np.array_equal(y.cpu().numpy()[0], want_y), (quality, optimize)
            assert nc == 1 or np.array_equal(c.cpu().numpy()[0], want_c), (quality, optimize)
            # the pixels
            fb, frames = poisoned((1, H, W, 3), torch.uint8)
            o.jpeg_rgb(y, c, H, W, layout=layout, out=frames)
            assert np.array_equal(frames.cpu().numpy()[0], want_rgb), (quality, optimize)
            assert intact((yb, y), (fb, frames)) and (nc == 1 or intact((cb, c)))


@pytest.mark.parametrize("name", list(L.LAYOUTS))
def test_segments_of_restart_files_and_whole_frames_share_a_launch(name):
    """two frames of one table set: one without restart markers (one segment), one cut every 2 MCUs (a short last interval)"""
    o, layout, (H, W) = ops(), L.LAYOUTS[name], (17, 33)
    mr, mc = L.grid(H, W, layout)
    _, (f0, want0, *_) = case(name, H, W, 90, False)
    _, (f1, want1, *_) = case(name, H, W, 90, False, (("restart_marker_blocks", 2),))
    assert f1["ri"] == 2 and len(f1["parts"]) == -(-mr * mc // 2) and f0["specs"] == f1["specs"] and np.array_equal(want0, want1)
    got, status = decode_segments(o, [(0, f0["parts"]), (2, f1["parts"])], f0["specs"], mr * mc, layout)
    assert len(status) == 1 + len(f1["parts"]) and not status.any()
    assert np.array_equal(got[0], want0) and np.array_equal(got[1], want1)


@pytest.mark.parametrize("name", list(L.LAYOUTS))
def test_pixel_kernels_on_planes_of_independent_bytes(name):
    """every filter tap and colour clamp at full range, padded samples that must not be read, coefficients no encoder makes, 3 frames"""
    o, layout, (n, H, W) = ops(), L.LAYOUTS[name], (3, 17, 33)
    nc, hs, vs = layout
    mr, mc = L.grid(H, W, layout)
    rng = np.random.default_rng(H * W + hs + vs + nc)
    y_host = rng.integers(0, 256, (n, mr * 8 * vs, mc * 8 * hs), dtype=np.uint8)
    c_host = rng.integers(0, 256, (n, 2, mr * 8, mc * 8), dtype=np.uint8) if nc == 3 else None
    dev_c = lambda: to_dev(c_host) if nc == 3 else None
    got = o.jpeg_rgb(to_dev(y_host), dev_c(), H, W, layout=layout).cpu().numpy()
    assert np.array_equal(got, L.to_rgb(y_host, c_host, H, W, layout))
    if nc == 3:
        c_host[:, :, -(-H // vs):], c_host[:, :, :, -(-W // hs):] = 0, 0         # behind the real chroma samples
        assert np.array_equal(o.jpeg_rgb(to_dev(y_host), dev_c(), H, W, layout=layout).cpu().numpy(), got)
    wild = rng.integers(-32768, 32768, (n, mr * mc, L.bpm(layout), 64)).astype(np.int16)
    quant = np.stack([np.full(64, v, np.uint16) for v in (255, 254, 253)])
    y, c = o.jpeg_idct(to_dev(wild), to_dev(quant), H, W, layout=layout)
    want_y, want_c = L.idct(wild, quant, H, W, layout)
    assert np.array_equal(y.cpu().numpy(), want_y) and (nc == 1 or np.array_equal(c.cpu().numpy(), want_c))


def test_layout_entries_refuse_what_is_not_built():
    o = ops()
    lib = o._lib.load()
    z = torch.zeros(4096, device=DEV, dtype=torch.uint8)
    p = o._ptr(z)
    for nc, hs, vs in ((3, 1, 2), (3, 4, 1), (4, 1, 1), (1, 2, 2), (2, 1, 1)):   # 4:4:0, 4:1:1, four components, ...
        assert lib.emo_jpeg_decode_bits(p, 4096, p, p, p, p, 1, 1, nc, hs, vs, o._stream()) != 0
        assert lib.emo_jpeg_decode_segments(p, 4096, p, p, p, p, p, 1, p, 1, nc, hs, vs, o._stream()) != 0
        assert lib.emo_jpeg_idct(p, p, p, p, 1, 8, 8, nc, hs, vs, o._stream()) != 0
        assert lib.emo_jpeg_rgb(p, p, p, 1, 8, 8, nc, hs, vs, o._stream()) != 0
    for H, W in ((8, 70000), (0, 8)):                                            # SOF0 holds 16 bits
        assert lib.emo_jpeg_idct(p, p, p, p, 1, H, W, 3, 2, 1, o._stream()) != 0
        assert lib.emo_jpeg_rgb(p, p, p, 1, H, W, 3, 2, 1, o._stream()) != 0
    with pytest.raises(AssertionError):
        o.jpeg_bpm((3, 1, 2))


# ------------------------------------------------------------------------------------------------------------------- truncated scans
@pytest.mark.parametrize("name", list(L.LAYOUTS))
def test_truncated_scans_report_and_return(name):
    """an error status from bounded reads: the frame's blocks behind the cut are zeroed, its neighbours decode"""
    o, layout, (H, W) = ops(), L.LAYOUTS[name], (38, 70)
    mr, mc = L.grid(H, W, layout)
    data, (f, want, *_) = case(name, H, W, 90, False)
    whole = f["parts"][0]
    cut = whole[:len(whole) * 2 // 3]
    got, status = decode_bits(o, [whole, cut, whole], f["specs"], mr * mc, layout)
    assert list(status) == [D.OK, D.PAST_END, D.OK] and np.array_equal(got[0], want) and np.array_equal(got[2], want)
    blocks = got[1].reshape(-1, 64)
    done = int(blocks.any(axis=1).nonzero()[0].max()) + 1                        # the blocks in front of the cut are there, nothing behind
    assert 0 < done < len(blocks) and np.array_equal(blocks[:done - 1], want.reshape(-1, 64)[:done - 1]) and not blocks[done:].any()
    got, status = decode_segments(o, [(0, [whole]), (0, [cut]), (0, [whole])], f["specs"], mr * mc, layout)
    assert list(status) == [D.OK, D.PAST_END, D.OK] and np.array_equal(got[0], want) and np.array_equal(got[2], want)
    # the same through decode_mjpeg: a ValueError that names the frame and the reason
    sos = data.index(b"\xFF\xDA")
    head = data[:sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")]
    body = data[len(head):-2]
    damaged = head + body[:len(body) * 2 // 3] + b"\xFF\xD9"
    with pytest.raises(ValueError, match="frame 1 does not decode: the scan ends before the frame's last block"):
        V.decode_mjpeg([data, damaged, data])
    assert np.array_equal(V.decode_mjpeg([data, data]).cpu().numpy()[1], L.pillow_decode(data))      # and the card is well


# ------------------------------------------------------------------------------------------------------------------- against Pillow
@pytest.mark.parametrize("name", list(L.LAYOUTS))
def test_decode_mjpeg_equals_pillow(name):
    for H, W in L.SIZES[name]:
        for quality, optimize in ((10, True), (90, False), (100, True)):
            data, _ = case(name, H, W, quality, optimize)
            got = V.decode_mjpeg([data])
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (1, H, W, 3)
            assert np.array_equal(got.cpu().numpy()[0], L.pillow_decode(data)), (H, W, quality, optimize)
    # with restart intervals, and frames with and without in one call
    for H, W in L.SIZES[name][-2:]:
        files = [case(name, H, W, 90, False, tuple(kw.items()))[0] for kw in RESTARTS]
        assert [V.parse_jpeg(d, restart=True, layouts=True).restart > 0 for d in files] == [False, True, True, True]
        for d in files[1:]:
            assert np.array_equal(V.decode_mjpeg([d]).cpu().numpy()[0], L.pillow_decode(d)), (H, W)
        assert np.array_equal(V.decode_mjpeg(files).cpu().numpy(), np.stack([L.pillow_decode(d) for d in files])), (H, W)


def test_decode_mjpeg_on_layouts_that_were_refused():
    """what `decode_mjpeg` raised "sampling factors 2x1 / 1x1 / 1x1" and the like on"""
    for name in ("4:2:2", "4:4:4", "grey"):
        data, _ = case(name, 38, 70, 90, False)
        assert np.array_equal(V.decode_mjpeg([data]).cpu().numpy()[0], L.pillow_decode(data)), name


def test_decode_mjpeg_mixes_layouts_in_one_call():
    H, W = 38, 70
    names = ["4:2:0", "4:2:2", "4:4:4", "grey", "4:2:2", "4:2:0", "grey", "4:4:4"]
    files = [case(name, H, W, (90, 10)[i % 2], i >= 4)[0] for i, name in enumerate(names)]
    got = V.decode_mjpeg(files)
    assert tuple(got.shape) == (len(files), H, W, 3)
    assert np.array_equal(got.cpu().numpy(), np.stack([L.pillow_decode(d) for d in files]))
    grey = got[3].cpu().numpy()
    assert np.array_equal(grey[..., 0], grey[..., 1]) and np.array_equal(grey[..., 0], grey[..., 2])
    with pytest.raises(ValueError, match="frame 1 is 17 x 33"):
        V.decode_mjpeg([files[0], case("4:4:4", 17, 33, 90, False)[0]])


def test_decode_mjpeg_with_three_quantisers():
    pic = D.picture(38, 70, 9)
    for name in ("4:4:4", "4:2:2", "4:2:0"):
        for optimize in (False, True):
            data = L.three_quantiser_file(pic, name, optimize)
            assert np.array_equal(V.decode_mjpeg([data]).cpu().numpy()[0], L.pillow_decode(data)), (name, optimize)


def test_decode_mjpeg_420_with_one_and_with_two_chrominance_quantisers():
    """4:2:0 with Cb and Cr on one quantiser had entries of its own once; it and 4:2:0 with three quantisers now share them.  Two groups
    of 2 x 24 x 40 frames (one and a half MCU rows, two and a half MCU columns: the padded edge and the chroma clamp) in one call, un-cut
    (emo_jpeg_decode_bits; consecutive members, a slice copy) and cut every 2 MCUs (emo_jpeg_decode_segments; alternating members, an
    index scatter), against the restatement byte for byte"""
    H, W = 24, 40
    pics = [D.picture(H, W, seed) for seed in (3, 4)]
    for kw, order in ((dict(), (0, 1, 2, 3)), (dict(restart_marker_blocks=2), (0, 2, 1, 3))):
        files = [L.pillow_file(p, "4:2:0", 90, False, **kw) for p in pics] + [L.three_quantiser_file(p, "4:2:0", False, **kw) for p in pics]
        files = [files[i] for i in order]
        parsed = [V.parse_jpeg(d, restart=True, layouts=True) for d in files]
        assert all(p.layout.key == (3, 2, 2) and (p.height, p.width, p.mcus) == (H, W, 6) and p.restart == (2 if kw else 0) for p in parsed)
        equal = [np.array_equal(p.quants[1], p.quants[2]) for p in parsed]
        assert equal == [i < 2 for i in order] and len({p.table_key() for p in parsed}) == 2
        got = V.decode_mjpeg(files)
        assert tuple(got.shape) == (4, H, W, 3)
        assert np.array_equal(got.cpu().numpy(), np.stack([L.decode(d) for d in files])), kw


# ------------------------------------------------------------------------------------------------------------------- still images
def test_read_image(tmp_path):
    from PIL import Image
    for name in L.LAYOUTS:
        data, _ = case(name, 38, 70, 90, True)
        path = tmp_path / f"still_{name.replace(':', '')}.jpg"
        path.write_bytes(data)
        for src in (data, str(path), path):
            got = V.read_image(src)
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (38, 70, 3)
            assert np.array_equal(got.cpu().numpy(), L.pillow_decode(data)), name
    data, _ = case("4:2:2", 38, 70, 90, False)
    for size, resample, pil in (((64, 64), "bicubic", Image.BICUBIC), ((40, 24), "bilinear", Image.BILINEAR)):
        want = np.array(Image.open(io.BytesIO(data)).convert("RGB").resize(size, pil))
        got = V.read_image(data, size=size, resample=resample)
        assert tuple(got.shape) == (size[1], size[0], 3) and np.array_equal(got.cpu().numpy(), want), size
    assert np.array_equal(V.read_image(data, size=(64, 64)).cpu().numpy(), np.array(Image.open(io.BytesIO(data)).convert("RGB").resize((64, 64))))
    buf = io.BytesIO()
    Image.fromarray(D.picture(38, 70, 1)).save(buf, format="JPEG", quality=90, progressive=True)
    with pytest.raises(ValueError, match="read_image: parse_jpeg: a progressive"):
        V.read_image(buf.getvalue())


@pytest.fixture(scope="module")
def pipe():
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    from tests import cases
    from tests.test_gpu_unet import build
    from tests.test_gpu_vae import SMALL, build as build_vae
    return EMOAnimationPipeline(vae=build_vae(SMALL, torch.float32)[0], unet=build(cases.TINY_MOTION, torch.float32), scheduler=DDIMScheduler())


def pillow_source_image(path, width, height):
    """what _source_image_rgb did with every path before: EMOAnimationPipeline.py:686-689"""
    from PIL import Image
    return np.array(Image.open(path).convert("RGB").resize((width, height)))


def test_source_image_from_a_still_jpeg_stays_on_the_device(pipe, tmp_path):
    from PIL import Image
    pic = D.picture(96, 120, 4)
    for name in L.LAYOUTS:
        path = str(tmp_path / f"portrait_{name.replace(':', '')}.JPG")
        open(path, "wb").write(L.pillow_file(pic, name, 90, True))
        for width, height in ((64, 64), (120, 96)):                              # resized, and at size
            rgb = pipe._source_image_rgb(path, width, height)
            assert torch.is_tensor(rgb) and rgb.is_cuda and rgb.dtype == torch.uint8
            assert np.array_equal(rgb.cpu().numpy(), pillow_source_image(path, width, height)), (name, width, height)
    path = str(tmp_path / "portrait_422.JPG")
    from_path = pipe._source_image_latents(path, 64, 64)
    from_array = pipe._source_image_latents(pillow_source_image(path, 64, 64), 64, 64)
    assert from_path.is_cuda and tuple(from_path.shape) == (1, 4, 8, 8) and float(from_path.abs().max()) > 0
    assert torch.allclose(from_path, from_array.to(from_path.device), rtol=1e-3, atol=1e-4), float((from_path - from_array.to(from_path.device)).abs().max())
    with pytest.raises(ValueError, match="multiple of 8"):
        pipe._source_image_rgb(path, 60, 64)
    # what parse_jpeg refuses, and every other format, is Pillow's as before: a host array
    prog, png = str(tmp_path / "progressive.jpg"), str(tmp_path / "portrait.png")
    Image.fromarray(pic).save(prog, format="JPEG", quality=90, progressive=True)
    Image.fromarray(pic).save(png)
    for other in (prog, png):
        rgb = pipe._source_image_rgb(other, 64, 64)
        assert isinstance(rgb, np.ndarray) and np.array_equal(rgb, pillow_source_image(other, 64, 64))
