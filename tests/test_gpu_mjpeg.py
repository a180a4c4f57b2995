"""GPU tests of the Motion-JPEG writer: emo_jpeg_blocks / emo_jpeg_count_bits / emo_jpeg_emit_bits (csrc/video_out.hip) against the float64
restatement in tests/mjpeg_ref.py, encode_mjpeg through Pillow's decoder, and the way from latents to an `.avi` file with sound
(AutoencoderKL.decode_video(output="uint8") -> encode_mjpeg -> write_avi; `__call__(save_path=)`).

Coefficients: the kernel works in f32, the restatement in f64.  A coefficient is a sum of 64 products of values <= 1024 taken as two
8-term passes; the f32 error of that is about 1e-3 of a quantisation step at worst (q = 1), so the two may round differently only where
the f64 quotient lies within 0.01 of a tie (ten times that), and then by one.  Everywhere else they are equal.
Bits: the restatement's serial entropy coder, run on the DEVICE's coefficients, gives every block's bit count and every byte of the stream.
PSNR: the per-(content, quality) gates of tests/test_video_io_host.py, measured there on these same frames."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from emote_hack_amd import video_io as V
from emote_hack_amd.synth import seeded_randn
from tests import cases
from tests import mjpeg_ref as R
from tests.test_gpu_kernels import DEV, ops
from tests.test_video_io_host import DEFICIT_DB, GATE_MARGIN_DB, WORST_GATE_DB, check_decodes_within_gate

pytestmark = pytest.mark.gpu
TIE_WINDOW = 0.01
POISON = 0xA5


def device_tables(quality):
    t = V.jpeg_tables(quality)
    return t, torch.from_numpy(t.quant.copy()).to(DEV), torch.from_numpy(t.huff.astype(np.int32)).to(DEV)


def emit_into_poisoned_buffer(o, coefs, huff, counts):
    """what encode_streams does, into a buffer whose every byte behind the last stream byte holds POISON -> (buffer, starts, bits, total)"""
    ends = torch.cumsum(counts, dim=1, dtype=torch.int64)
    bits = ends[:, -1].cpu().numpy()
    nbytes = (bits + 7) // 8
    starts = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    total = int(nbytes.sum())
    words = (total + 3) // 4 * 4
    buf = torch.full((words + 64,), POISON, device=DEV, dtype=torch.uint8)
    buf[:total] = 0
    offsets = (ends - counts + torch.from_numpy(starts * 8).to(DEV)[:, None]).contiguous()
    o.jpeg_emit_bits(coefs, huff, offsets, buf[:words])
    return buf.cpu().numpy(), starts, bits, total


@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("n,H,W", R.SHAPES)
def test_kernels_against_the_restatement(n, H, W, content):
    o = ops()
    frames = R.make_frames(content, n, H, W)
    dev_frames = torch.from_numpy(frames).to(DEV)
    for quality in R.QUALITIES:
        what = f"{content} {n}x{H}x{W} q{quality}"
        t, quant, huff = device_tables(quality)
        coefs = o.jpeg_blocks(dev_frames, quant)
        mr, mc = R.n_mcus(H, W)
        assert coefs.dtype == torch.int16 and tuple(coefs.shape) == (n, mr * mc, 6, 64)
        got = coefs.cpu().numpy()
        want, quot = R.blocks(frames, t.quant)
        diff = got.astype(np.int64) - want
        tie_distance = np.abs(np.abs(quot - np.floor(quot)) - 0.5)
        off = diff != 0
        print(f"{what}: {int(off.sum())} of {off.size} coefficients differ, max |diff| {int(np.abs(diff).max())}, "
              f"their largest distance from a tie {float(tie_distance[off].max()) if off.any() else 0.0:.2e}")
        assert int(np.abs(diff).max()) <= 1, what
        assert not off.any() or float(tie_distance[off].max()) <= TIE_WINDOW, what
        # entropy coding, on the device's own coefficients
        counts = o.jpeg_count_bits(coefs, huff)
        assert counts.dtype == torch.int32 and tuple(counts.shape) == (n, mr * mc * 6)
        ref_counts, ref_streams, seen = R.entropy(got, t.huff)
        assert np.array_equal(counts.cpu().numpy(), ref_counts), what
        buf, starts, bits, total = emit_into_poisoned_buffer(o, coefs, huff, counts)
        for i, (stream, nbits) in enumerate(ref_streams):
            assert int(bits[i]) == nbits
            assert np.array_equal(buf[starts[i]:starts[i] + len(stream)], stream), (what, i)
        assert starts[-1] + len(ref_streams[-1][0]) == total and bool((buf[total:] == POISON).all()), what
        # what the frames are for
        if content == "flat":
            assert not (got[..., 1:] != 0).any() and not (got[:, 1:, :, 0] != got[:, :1, :, 0]).any()      # EOB only, zero DC differences
        if content == "noise" and quality == 100 and n > 1:
            assert seen["dc_category"] == 11 and seen["ac_category"] == 10 and int((buf[:total] == 0xFF).sum()) > 0
        if content == "impulses" and quality == 50 and n > 1:
            assert seen["zrl"] > 0
        # the product's path: the same bytes, framed, and Pillow decodes them
        jpegs = V.encode_mjpeg(dev_frames, quality)
        assert len(jpegs) == n
        for i, (stream, nbits) in enumerate(ref_streams):
            assert jpegs[i] == V.jpeg_header(H, W, quality) + V.finish_scan(stream, nbits), (what, i)
            check_decodes_within_gate(jpegs[i], frames[i], quality, DEFICIT_DB[content, quality] + GATE_MARGIN_DB, f"{what} #{i}")


def test_every_frame_restarts_the_dc_prediction():
    """three equal frames give three equal streams: the predictor is 0 at each frame's first MCU, whatever the previous frame ended on"""
    o = ops()
    one = R.make_frames("ramp", 1, 70, 38)
    frames = torch.from_numpy(np.concatenate([one, one, one])).to(DEV)
    a, b, c = V.encode_mjpeg(frames, 90)
    assert a == b == c and a == V.encode_mjpeg(frames[:1], 90)[0]
    five = V.encode_mjpeg(frames[None], 50)                                      # the (1, n, H, W, 3) of output_type="uint8"
    assert len(five) == 3 and five[0] == five[2] != a


def test_entry_point_refusals():
    from emote_hack_amd._lib import EmoHipError
    o = ops()
    t, quant, huff = device_tables(90)
    frames = torch.zeros(1, 8, 8, 3, device=DEV, dtype=torch.uint8)
    coefs = o.jpeg_blocks(frames, quant)
    counts = o.jpeg_count_bits(coefs, huff)
    offsets = (torch.cumsum(counts, 1, dtype=torch.int64) - counts).contiguous()
    with pytest.raises(EmoHipError, match="multiple of 4"):
        o.jpeg_emit_bits(coefs, huff, offsets, torch.zeros(30, device=DEV, dtype=torch.uint8))
    with pytest.raises(EmoHipError, match="multiple of 4"):
        o.jpeg_emit_bits(coefs, huff, offsets, torch.zeros(33, device=DEV, dtype=torch.uint8)[1:])       # misaligned
    with pytest.raises(EmoHipError):
        o.jpeg_blocks(torch.zeros(1, 8, 70000, 3, device=DEV, dtype=torch.uint8), quant)                 # SOF0 holds 16 bits
    with pytest.raises(EmoHipError):
        V.encode_mjpeg(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))                                       # host frames: no CPU path
    # offsets that point outside the buffer write nothing at all
    buf = torch.full((64,), POISON, device=DEV, dtype=torch.uint8)
    o.jpeg_emit_bits(coefs, huff, offsets + 8 * 64, buf)
    o.jpeg_emit_bits(coefs, huff, offsets - 8 * 4096, buf)
    assert bool((buf == POISON).all())


def sine(n, rate, hz=440.0, channels=1):
    t = np.arange(n, dtype=np.float64) / rate
    return np.stack([0.6 * np.sin(2 * np.pi * hz * (c + 1) * t) for c in range(channels)], axis=1).astype(np.float32)


def test_latents_to_an_avi_file_with_sound(tmp_path):
    from tests.test_gpu_vae import SMALL, build
    m, _ = build(SMALL, torch.float32)
    lat = 0.2 * seeded_randn((1, 4, 5, 8, 8), 9)
    frames = m.decode_video(lat.to(DEV), frames_per_call=2, output="uint8")      # (1, 5, 64, 64, 3)
    jpegs = V.encode_mjpeg(frames, 90)
    audio = sine(16000 * 5 // 25, 16000, channels=2)
    path = tmp_path / "clip.avi"
    V.write_avi(path, jpegs, 64, 64, 25, audio=(audio, 16000))
    got, fps, (pcm, rate) = V.read_avi(path)
    assert len(got) == 5 and got == jpegs and fps == 25 and rate == 16000 and np.array_equal(pcm, V.pcm16(audio))
    host = frames[0].cpu().numpy()
    assert len(np.unique(host)) > 16
    for i, j in enumerate(got):
        check_decodes_within_gate(j, host[i], 90, WORST_GATE_DB, f"decoded clip #{i}")
    back = V.video2images(path, step=2, length=2, start=1)                       # frames 1 and 3
    assert len(back) == 2 and np.array_equal(back[0], R.decode(jpegs[1])) and np.array_equal(back[1], R.decode(jpegs[3]))


def test_reference_surface_writes_grids(tmp_path):
    videos = torch.rand(3, 3, 4, 10, 6, generator=torch.Generator().manual_seed(3))
    path = tmp_path / "sub" / "grid.avi"                                         # the directory is made (util.py:32)
    V.save_videos_grid(videos, str(path), n_rows=2, fps=8)
    jpegs, fps, audio = V.read_avi(path)
    assert len(jpegs) == 4 and fps == 8 and audio is None
    want = V.make_grid_u8(videos, n_rows=2).numpy()
    assert want.shape == (4, 26, 18, 3)
    for i, j in enumerate(jpegs):
        check_decodes_within_gate(j, want[i], 90, WORST_GATE_DB, f"grid #{i}")
    path2 = tmp_path / "frames.avi"
    V.images2video([f for f in want], str(path2))
    jpegs2, fps2, _ = V.read_avi(path2)
    assert fps2 == 8 and jpegs2 == jpegs                                         # images2video's default rate; the same frames, the same bytes
    assert [f.shape for f in V.video2images(path2)] == [(26, 18, 3)]             # [0::4][:16] of four frames


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


def test_call_save_path_writes_the_clip_with_its_sound(env, tmp_path):
    pipe, kw = env["pipe"], env["kw"]
    samples = sine(16000, 16000)[:, 0]                                           # one second, mono
    path = tmp_path / "clip.avi"
    plain = pipe("", output_type="uint8", interpolation_factor=2, **kw).videos
    got = pipe("", output_type="uint8", interpolation_factor=2, fps=25, audio=(samples, 16000), save_path=str(path), **kw).videos
    assert torch.equal(got, plain)                                               # the return value is what it was
    n_frames = (F_TOT - 1) * 2 + 1
    assert tuple(got.shape) == (1, n_frames, 128, 128, 3)
    jpegs, fps, (pcm, rate) = V.read_avi(path)
    assert len(jpegs) == n_frames and fps == 50 and rate == 16000
    n_samples = math.floor(Fraction(n_frames * 16000, 50) + Fraction(1, 2))      # the clip's duration
    assert pcm.shape == (n_samples, 1) and np.array_equal(pcm[:, 0], V.pcm16(samples)[:n_samples, 0])
    assert jpegs == V.encode_mjpeg(got, 90)
    host = got[0].cpu().numpy()
    for i in (0, n_frames - 1):
        check_decodes_within_gate(jpegs[i], host[i], 90, WORST_GATE_DB, f"call #{i}")
    # latents returned, a lower quality, stereo sound that starts late and ends before the clip does
    path2 = tmp_path / "clip2.avi"
    stereo = sine(3000, 8000, channels=2)
    lat = pipe("", output_type="latent", fps=(25, 1), audio=(stereo, 8000), audio_start=Fraction(1, 4), save_path=path2, save_quality=50, **kw).videos
    assert torch.equal(lat, pipe("", output_type="latent", **kw).videos)
    jpegs2, fps2, (pcm2, rate2) = V.read_avi(path2)
    assert len(jpegs2) == F_TOT and fps2 == 25 and rate2 == 8000
    assert np.array_equal(pcm2, V.pcm16(stereo)[2000:])                          # 4 / 25 s would be 1280 samples; 1000 are left
    assert jpegs2 == V.encode_mjpeg(env["vae"].decode_video(lat, output="uint8"), 50)
    assert sum(map(len, jpegs2)) * n_frames < sum(map(len, jpegs)) * F_TOT       # quality 50 is the smaller file per frame
