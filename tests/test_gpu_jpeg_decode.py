"""GPU tests of the Motion-JPEG reader: emo_jpeg_decode_bits / emo_jpeg_idct / emo_jpeg_rgb (csrc/video_in.hip) at 4:2:0 against the
numpy restatement in tests/jpeg_decode_ref.py (which tests/test_jpeg_decode_host.py holds to Pillow's decoder byte for byte), decode_mjpeg
and read_video against Pillow's decoder itself, and the pipeline taking its control frames and its source image from a clip.

Everything is integer arithmetic, so every comparison is an equality.  Every output a kernel writes is the front of a larger buffer whose
tail holds a poison value that must come back untouched."""
import numpy as np
import pytest
import torch

from emote_hack_amd import video_io as V
from emote_hack_amd.synth import seeded_randn
from tests import cases
from tests import jpeg_decode_ref as D
from tests import mjpeg_ref as R
from tests.test_gpu_kernels import DEV, ops

pytestmark = pytest.mark.gpu
GUARD = 256
POISON = {torch.uint8: 0xA5, torch.int16: 0x5A5A, torch.int32: 0x5A5A5A5A}
PIXEL_SHAPES = [(1, 8, 8), (1, 5, 9), (1, 9, 5), (2, 24, 40), (3, 70, 38)]      # smaller than an MCU (chroma plane 4 x 4) ... odd tails


def poisoned(shape, dtype):
    """(the whole buffer, its front as a tensor of `shape`): what is behind the front holds POISON[dtype]"""
    numel = int(np.prod(shape))
    buf = torch.full((numel + GUARD,), POISON[dtype], device=DEV, dtype=dtype)
    return buf, buf[:numel].view(shape)


def intact(*bufs_and_fronts):
    return all(bool((buf[front.numel():] == POISON[buf.dtype]).all()) for buf, front in bufs_and_fronts)


def device_decode_tables(specs):
    return torch.from_numpy(np.stack([V.huffman_decode_table(*s) for s in specs])).to(DEV)


def decode_bits(o, scan, offsets, specs, n_mcu):
    """ops.jpeg_decode_bits into poisoned buffers -> (coefficients, status) on the host"""
    n = len(offsets) - 1
    cb, coefs = poisoned((n, n_mcu, 6, 64), torch.int16)
    sb, status = poisoned((n,), torch.int32)
    scan = scan if torch.is_tensor(scan) else torch.from_numpy(np.concatenate([scan, np.zeros(-len(scan) % 4 or (0 if len(scan) else 4), np.uint8)])).to(DEV)
    o.jpeg_decode_bits(scan, torch.from_numpy(np.asarray(offsets, np.int64)).to(DEV), device_decode_tables(specs), n_mcu, out=coefs, status=status)
    torch.cuda.synchronize()
    assert intact((cb, coefs), (sb, status))
    return coefs.cpu().numpy(), status.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------- entropy decoding
@pytest.mark.parametrize("content", R.CONTENTS)
def test_decode_bits_returns_what_the_device_encoder_was_given(content):
    o = ops()
    seen = {q: dict(dc=0, ac=0, ff=0, zrl_runs=0, eob_only=True) for q in R.QUALITIES}
    for n, H, W in R.SHAPES:
        dev_frames = torch.from_numpy(R.make_frames(content, n, H, W)).to(DEV)
        for quality in R.QUALITIES:
            t = V.jpeg_tables(quality)
            coefs = o.jpeg_blocks(dev_frames, torch.from_numpy(t.quant.copy()).to(DEV))
            stream, starts, bits = V.encode_streams(dev_frames, quality)
            offsets = np.concatenate([starts, [starts[-1] + (bits[-1] + 7) // 8]])
            got, status = decode_bits(o, stream, offsets, t.specs, coefs.shape[1])
            want = coefs.cpu().numpy()
            assert not status.any(), (content, n, H, W, quality, status)
            assert np.array_equal(got, want), (content, n, H, W, quality)
            s = seen[quality]
            dc = want[:, :, :4, 0].reshape(n, -1).astype(np.int64)
            s["dc"] = max(s["dc"], int(np.abs(np.diff(dc, axis=1, prepend=0)).max()))
            s["ac"] = max(s["ac"], int(np.abs(want[..., 1:].astype(np.int64)).max()))
            s["ff"] += int((stream.cpu().numpy()[:int(offsets[-1])] == 0xFF).sum())
            nz = want != 0
            nz[..., 0] = True                                                   # the longest zero run in front of a non-zero AC term
            idx = np.where(nz, np.arange(64), -1)
            gaps = np.diff(np.maximum.accumulate(idx, axis=-1), axis=-1)
            s["zrl_runs"] += int((gaps > 16).sum())
            s["eob_only"] &= not want[..., 1:].any()
    # what the frames are for
    if content == "noise":
        assert seen[100]["dc"] >= 1024 and seen[100]["ac"] >= 512 and seen[100]["ff"] > 0      # DC category 11, AC category 10, FF bytes
    if content == "impulses":
        assert seen[50]["zrl_runs"] > 0
    if content == "flat":
        assert all(s["eob_only"] for s in seen.values())


def test_every_frame_restarts_the_dc_prediction():
    o = ops()
    one = R.make_frames("ramp", 1, 70, 38)
    frames = torch.from_numpy(np.concatenate([one, one, one])).to(DEV)
    t = V.jpeg_tables(90)
    stream, starts, bits = V.encode_streams(frames, 90)
    offsets = np.concatenate([starts, [starts[-1] + (bits[-1] + 7) // 8]])
    got, status = decode_bits(o, stream, offsets, t.specs, ops().jpeg_mcus(70, 38))
    assert not status.any() and np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2]) and got[0, :, :, 0].any()
    assert np.array_equal(got, o.jpeg_blocks(frames, torch.from_numpy(t.quant.copy()).to(DEV)).cpu().numpy())


def test_streams_longer_than_the_staging_window():
    """128 x 96 noise at quality 100 codes about 15 KB per frame: the walker passes many windows and many flushes, and picks up in the
    middle of a byte each time"""
    o = ops()
    n, H, W = 2, 96, 128
    frames = torch.from_numpy(R.make_frames("noise", n, H, W)).to(DEV)
    t = V.jpeg_tables(100)
    stream, starts, bits = V.encode_streams(frames, 100)
    assert int(bits.min()) > 8 * 3 * 4096
    offsets = np.concatenate([starts, [starts[-1] + (bits[-1] + 7) // 8]])
    got, status = decode_bits(o, stream, offsets, t.specs, o.jpeg_mcus(H, W))
    assert not status.any() and np.array_equal(got, o.jpeg_blocks(frames, torch.from_numpy(t.quant.copy()).to(DEV)).cpu().numpy())


def test_damaged_scans_report_and_return():
    o = ops()
    n, H, W = 3, 70, 38
    t = V.jpeg_tables(90)
    n_mcu = o.jpeg_mcus(H, W)
    want, _ = R.blocks(R.make_frames("ramp", n, H, W), t.quant)
    scans = [np.frombuffer(s.tobytes(), np.uint8)[:(b + 7) // 8] for s, b in R.entropy(want, t.huff)[1]]
    ends = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    # a scan cut in half, between two good ones
    parts = [scans[0], scans[1][:len(scans[1]) // 2], scans[2]]
    got, status = decode_bits(o, np.concatenate(parts), ends(parts), t.specs, n_mcu)
    assert list(status) == [D.OK, D.PAST_END, D.OK] and np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    done = int(got[1].reshape(-1, 64).any(axis=1).nonzero()[0].max()) + 1       # the blocks in front of the cut are there, nothing behind
    assert 0 < done < n_mcu * 6 and np.array_equal(got[1].reshape(-1, 64)[:done - 1], want[1].reshape(-1, 64)[:done - 1])
    # sixteen 1-bits are no code of any table (Annex C never assigns the all-ones code)
    parts = [scans[0], np.concatenate([np.array([0xFF, 0xFF], np.uint8), scans[1]]), scans[2]]
    got, status = decode_bits(o, np.concatenate(parts), ends(parts), t.specs, n_mcu)
    assert list(status) == [D.OK, D.BAD_CODE, D.OK] and not got[1].any() and np.array_equal(got[2], want[2])
    # byte offsets in which the middle frame is empty
    parts = [scans[0], scans[2]]
    e = ends(parts)
    got, status = decode_bits(o, np.concatenate(parts), [e[0], e[1], e[1], e[2]], t.specs, n_mcu)
    assert list(status) == [D.OK, D.PAST_END, D.OK] and not got[1].any() and np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    # four ZRLs and a coefficient: the run leaves the block
    code, length = V.huffman_codes(*V.HUFFMAN_SPECS[1])
    bits = "00" + 4 * format(int(code[0xF0]), f"0{int(length[0xF0])}b") + format(int(code[0x01]), f"0{int(length[0x01])}b") + "1"
    run = np.packbits(np.array([int(b) for b in bits + "1" * (-len(bits) % 8)], np.uint8))
    got, status = decode_bits(o, run, [0, len(run)], V.HUFFMAN_SPECS, 1)
    assert list(status) == [D.BAD_RUN] and not got.any()
    # the same through decode_mjpeg: a ValueError that names the frame and the reason, no frames
    head, good = V.jpeg_header(H, W, 90), [V.finish_scan(s, 8 * len(s)) for s in scans]
    half = scans[1][:len(scans[1]) // 2]
    for damaged, says in ((V.finish_scan(half, 8 * len(half)), "frame 1 does not decode: the scan ends"),
                          (V.finish_scan(np.concatenate([np.array([0xFF, 0xFF], np.uint8), scans[1]]), 8 * len(scans[1]) + 16),
                           "frame 1 does not decode: a code the Huffman table does not define"),
                          (b"\xFF\xD9", "frame 1 does not decode: the scan ends")):
        with pytest.raises(ValueError, match=says):
            V.decode_mjpeg([head + good[0], head + damaged, head + good[2]])
    with pytest.raises(ValueError, match="frame 1 is 16 x 16"):
        V.decode_mjpeg([head + good[0], V.jpeg_header(16, 16, 90) + b"\xFF\xD9"])
    assert np.array_equal(V.decode_mjpeg([head + good[0]]).cpu().numpy()[0], R.decode(head + good[0]))      # and the card is well


# ------------------------------------------------------------------------------------------------------------------- pixel kernels
@pytest.mark.parametrize("n,H,W", PIXEL_SHAPES)
def test_pixel_kernels_equal_the_restatement(n, H, W):
    o = ops()
    mr, mc = R.n_mcus(H, W)
    for content in R.CONTENTS:
        for quality in R.QUALITIES:
            t = V.jpeg_tables(quality)
            coefs, _ = R.blocks(R.make_frames(content, n, H, W), t.quant)
            yb, y = poisoned((n, mr * 16, mc * 16), torch.uint8)
            cb, c = poisoned((n, 2, mr * 8, mc * 8), torch.uint8)
            o.jpeg_idct(torch.from_numpy(np.ascontiguousarray(coefs)).to(DEV), torch.from_numpy(t.quant[[0, 1, 1]]).to(DEV), H, W, out_y=y, out_c=c)
            want_y, want_c = D.idct(coefs, t.quant, H, W)
            assert np.array_equal(y.cpu().numpy(), want_y) and np.array_equal(c.cpu().numpy(), want_c), (content, quality)
            fb, frames = poisoned((n, H, W, 3), torch.uint8)
            o.jpeg_rgb(y, c, H, W, out=frames)
            assert np.array_equal(frames.cpu().numpy(), D.h2v2_rgb(want_y, want_c, H, W)), (content, quality)
            assert intact((yb, y), (cb, c), (fb, frames))
    # planes of independent bytes: every filter tap and colour clamp at full range, and padded samples that must not be read
    rng = np.random.default_rng(H * W)
    y_host, c_host = rng.integers(0, 256, (n, mr * 16, mc * 16), dtype=np.uint8), rng.integers(0, 256, (n, 2, mr * 8, mc * 8), dtype=np.uint8)
    got = o.jpeg_rgb(torch.from_numpy(y_host).to(DEV), torch.from_numpy(c_host).to(DEV), H, W).cpu().numpy()
    assert np.array_equal(got, D.h2v2_rgb(y_host, c_host, H, W))
    ch, cw = (H + 1) // 2, (W + 1) // 2
    c_host[:, :, ch:], c_host[:, :, :, cw:] = 0, 0
    again = o.jpeg_rgb(torch.from_numpy(y_host).to(DEV), torch.from_numpy(c_host).to(DEV), H, W).cpu().numpy()
    assert np.array_equal(again, got)
    # coefficients no encoder makes: some byte comes out, the same one the wrapping restatement gives
    wild = rng.integers(-32768, 32768, (n, mr * mc, 6, 64)).astype(np.int16)
    quant = np.full((2, 64), 255, np.uint16)
    y, c = o.jpeg_idct(torch.from_numpy(wild).to(DEV), torch.from_numpy(quant[[0, 1, 1]]).to(DEV), H, W)
    want_y, want_c = D.idct(wild, quant, H, W)
    assert np.array_equal(y.cpu().numpy(), want_y) and np.array_equal(c.cpu().numpy(), want_c)


def test_entry_point_refusals():
    from emote_hack_amd._lib import EmoHipError
    o = ops()
    tables = device_decode_tables(V.HUFFMAN_SPECS)
    offsets = torch.zeros(2, device=DEV, dtype=torch.int64)
    with pytest.raises(EmoHipError, match="multiple of 4"):
        o.jpeg_decode_bits(torch.zeros(30, device=DEV, dtype=torch.uint8), offsets, tables, 1)
    with pytest.raises(EmoHipError, match="multiple of 4"):
        o.jpeg_decode_bits(torch.zeros(33, device=DEV, dtype=torch.uint8)[1:], offsets, tables, 1)
    lib = o._lib.load()
    z = torch.zeros(4096, device=DEV, dtype=torch.uint8)
    for H, W in ((8, 70000), (70000, 8), (0, 8)):                                # SOF0 holds 16 bits
        assert lib.emo_jpeg_idct(o._ptr(z), o._ptr(z), o._ptr(z), o._ptr(z), 1, H, W, 3, 2, 2, o._stream()) != 0
        assert lib.emo_jpeg_rgb(o._ptr(z), o._ptr(z), o._ptr(z), 1, H, W, 3, 2, 2, o._stream()) != 0
    with pytest.raises(EmoHipError):
        V.decode_mjpeg([V.jpeg_header(16, 16, 90) + b"\xFF\xD9"], device="cpu")   # no host decoder


# ------------------------------------------------------------------------------------------------------------------- against Pillow
def test_decode_mjpeg_equals_pillow():
    n, H, W = 3, 70, 38
    for content in ("ramp", "noise"):
        frames = R.make_frames(content, n, H, W)
        for quality in R.QUALITIES:
            ours = V.encode_mjpeg(torch.from_numpy(frames).to(DEV), quality)
            got = V.decode_mjpeg(ours)
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (n, H, W, 3)
            assert np.array_equal(got.cpu().numpy(), np.stack([R.decode(j) for j in ours])), (content, quality)
    # Pillow's own files, optimised: each brings its own Huffman tables
    for h, w in D.PILLOW_SIZES + [(40, 24)]:
        files = [D.pillow_file(D.picture(h, w, h * w + q), q, True) for q in D.PILLOW_QUALITIES]
        for f in files:
            assert np.array_equal(V.decode_mjpeg([f]).cpu().numpy()[0], R.decode(f)), (h, w)
    # one batch, two table sets out of order, and a third
    frames = R.make_frames("ramp", 3, 70, 38)
    q90, q50 = V.encode_mjpeg(torch.from_numpy(frames).to(DEV), 90), V.encode_mjpeg(torch.from_numpy(frames).to(DEV), 50)
    mixed = [q90[0], D.pillow_file(frames[1], 90, True), q50[1], q90[2], q50[0]]
    assert np.array_equal(V.decode_mjpeg(mixed).cpu().numpy(), np.stack([R.decode(j) for j in mixed]))


def test_read_video(tmp_path):
    n, H, W = 7, 40, 56
    frames = torch.from_numpy(np.stack([D.picture(H, W, i) for i in range(n)])).to(DEV)
    t = np.arange(16000 * n // 25, dtype=np.float64) / 16000
    audio = np.stack([0.6 * np.sin(2 * np.pi * 440.0 * (c + 1) * t) for c in range(2)], axis=1).astype(np.float32)
    path = tmp_path / "clip.avi"
    V.write_video(frames, str(path), 25, 90, audio=(audio, 16000))
    jpegs, _, _ = V.read_avi(path)
    got, fps, (pcm, rate) = V.read_video(path)
    assert got.is_cuda and tuple(got.shape) == (n, H, W, 3) and fps == 25 and rate == 16000 and np.array_equal(pcm, V.pcm16(audio))
    assert np.array_equal(got.cpu().numpy(), np.stack([R.decode(j) for j in jpegs]))
    for kw in (dict(step=2, length=2, start=1), dict(step=4, length=16, start=0), dict(step=1, length=3, start=5)):
        part, _, _ = V.read_video(path, **kw)
        assert np.array_equal(part.cpu().numpy(), np.stack(V.video2images(path, **kw))), kw
    with pytest.raises(ValueError, match="selects none"):
        V.read_video(path, start=n)


# ------------------------------------------------------------------------------------------------------------------- pipeline
F_TOT = 4
LOOP_KW = dict(num_inference_steps=2, guidance_scale=7.5, context_frames=4, context_stride=1, context_overlap=0, seed=0, output_type="latent")


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    from tests.test_gpu_controlnet import build_controlnet
    from tests.test_gpu_unet import build
    from tests.test_gpu_vae import SMALL, build as build_vae
    e = {}
    e["ref"] = build(cases.TINY, torch.float32, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    e["pipe"] = EMOAnimationPipeline(vae=build_vae(SMALL, torch.float32)[0], unet=build(cases.TINY_MOTION, torch.float32),
                                     controlnet=build_controlnet(torch.float32)[0], scheduler=DDIMScheduler())
    e["kw"] = dict(video_length=F_TOT, height=128, width=128, latents=seeded_randn((1, 4, F_TOT, 16, 16), 5).to(DEV),
                   text_embeddings=seeded_randn((2, 5, 32), 2), appearance_encoder=e["ref"], **LOOP_KW)
    e["path"] = str(tmp_path_factory.mktemp("clip") / "pose.avi")
    frames = torch.from_numpy(np.stack([D.picture(128, 128, 10 + i) for i in range(F_TOT + 1)])).to(DEV)
    V.write_video(frames, e["path"], 25, 90)
    e["decoded"] = np.stack([R.decode(j) for j in V.read_avi(e["path"])[0]])     # Pillow's frames of the same file
    return e


def test_pipeline_takes_control_frames_and_source_image_from_a_clip(env):
    pipe, kw, path, decoded = env["pipe"], env["kw"], env["path"], env["decoded"]
    ref_lat = seeded_randn((1, 4, 16, 16), 3)
    from_clip = pipe("", controlnet_condition=path, ref_image_latents=ref_lat, **kw).videos
    from_frames = pipe("", controlnet_condition=decoded[:F_TOT], ref_image_latents=ref_lat, **kw).videos
    assert torch.equal(from_clip, from_frames)
    other = pipe("", controlnet_condition=decoded[1:F_TOT + 1], ref_image_latents=ref_lat, **kw).videos
    assert not torch.equal(other, from_frames)                                   # and the frames matter
    src_clip = pipe("", controlnet_condition=decoded[:F_TOT], source_image=path, **kw).videos
    src_frame = pipe("", controlnet_condition=decoded[:F_TOT], source_image=decoded[0], **kw).videos
    assert torch.equal(src_clip, src_frame) and not torch.equal(src_clip, from_frames)


def test_pipeline_refuses_a_clip_it_would_have_to_resize_or_stretch(env):
    pipe, kw, path, decoded = env["pipe"], env["kw"], env["path"], env["decoded"]
    ref_lat = seeded_randn((1, 4, 16, 16), 3)
    small = dict(kw, height=64, width=64, latents=seeded_randn((1, 4, F_TOT, 8, 8), 5).to(DEV))
    with pytest.raises(ValueError, match="pass frames at size"):
        pipe("", controlnet_condition=path, ref_image_latents=seeded_randn((1, 4, 8, 8), 3), **small)
    with pytest.raises(ValueError, match="pass frames at size"):
        pipe("", controlnet_condition=decoded[:F_TOT, :64, :64], source_image=path, **small)
    long = dict(kw, video_length=8, latents=seeded_randn((1, 4, 8, 16, 16), 5).to(DEV))
    with pytest.raises(ValueError, match="holds 5 frames, 8 are needed"):
        pipe("", controlnet_condition=path, ref_image_latents=ref_lat, **long)
