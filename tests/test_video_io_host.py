"""CPU tests of emote_hack_amd/video_io.py: the JPEG tables, the framing of an entropy-coded stream into a file Pillow decodes, the AVI
container, the grid of save_videos_grid and every refusal.  The streams framed here come from tests/mjpeg_ref.py, the float64 restatement
of the kernels; tests/test_gpu_mjpeg.py puts the kernels' own streams through the same checks.

The PSNR gate.  A file framed here is decoded by Pillow and compared with the source frame; so is Pillow's own file of that frame at the
same quality (4:2:0, standard Huffman tables).  The restatement and libjpeg differ in the rounding of the DCT (libjpeg's is a scaled
integer transform) and of the chroma mean, which on frames this small moves the PSNR by tenths of a dB either way.  Measured here, the
restatement's DEFICIT = PSNR(Pillow's file) - PSNR(ours), the largest over the frames of tests/mjpeg_ref.SHAPES, in dB (where ours is
the better one the deficit is taken as 0):

    quality        10      50      90      100
    flat           0       0.706   0       0
    ramp           0.110   0.101   0.586   0.177
    noise          0.010   0.010   0.010   0.012
    impulses       0.067   0.050   0.011   0.002

The gate of a (content, quality) is that deficit plus 0.1 dB.  ZRL codes: an isolated saturated pixel on mid-grey has no DCT term above
127 * 0.49^2 = 31, under half of every quality-10 quantiser beyond the first few (K.1 * 5), so at quality 10 the impulse frames keep only
low-order terms and no run reaches 16; quality 50 is the lowest of the four at which they code ZRLs, and that is asserted."""
import io
import os
import struct
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from emote_hack_amd import video_io as V
from tests import mjpeg_ref as R

DEFICIT_DB = {
    ("flat", 10): 0.0, ("flat", 50): 0.706, ("flat", 90): 0.0, ("flat", 100): 0.0,
    ("ramp", 10): 0.110, ("ramp", 50): 0.101, ("ramp", 90): 0.586, ("ramp", 100): 0.177,
    ("noise", 10): 0.010, ("noise", 50): 0.010, ("noise", 90): 0.010, ("noise", 100): 0.012,
    ("impulses", 10): 0.067, ("impulses", 50): 0.050, ("impulses", 90): 0.011, ("impulses", 100): 0.002,
}
GATE_MARGIN_DB = 0.1
WORST_GATE_DB = max(DEFICIT_DB.values()) + GATE_MARGIN_DB          # for frames that are not in the table (a decoded clip)


def check_decodes_within_gate(jpeg, frame, quality, gate_db, what=""):
    """Pillow loads `jpeg` at the frame's size, and its PSNR against the frame is within gate_db of Pillow's own file's"""
    got = R.decode(jpeg)
    assert got.shape == frame.shape, (what, got.shape, frame.shape)
    ours, theirs = R.psnr(got, frame), R.psnr(R.decode(R.pillow_jpeg(frame, quality)), frame)
    print(f"{what}: PSNR ours {ours:.3f} dB, Pillow's {theirs:.3f} dB, gate {gate_db:.3f} dB")
    assert ours >= theirs - gate_db, (what, ours, theirs, gate_db)


# ------------------------------------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("quality", R.QUALITIES)
def test_tables_are_the_ones_in_pillows_baseline_file(quality):
    t = V.jpeg_tables(quality)
    quant, huff = R.jpeg_tables_in(R.pillow_jpeg(R.make_frames("noise", 1, 16, 16)[0], quality))
    assert sorted(quant) == [0, 1] and t.quant.dtype == np.uint16 and t.quant.shape == (2, 64)
    for i in range(2):
        assert np.array_equal(t.quant[i], quant[i]), (quality, i)                # natural order on both sides
    assert len(np.unique(t.quant[0])) > 1 or quality == 100
    assert sorted(huff) == sorted(V.HUFFMAN_IDS)
    for spec, ident in zip(t.specs, V.HUFFMAN_IDS):
        assert (tuple(spec[0]), bytes(spec[1])) == huff[ident], ident
    mine_q, mine_h = R.jpeg_tables_in(V.jpeg_header(16, 16, quality))            # ... and the product's header carries the same segments
    assert all(np.array_equal(mine_q[i], quant[i]) for i in range(2)) and mine_h == huff


def test_huffman_codes_follow_annex_c():
    t = V.jpeg_tables(50)
    entry = lambda tab, sym: (int(t.huff[tab, sym]) >> 16, int(t.huff[tab, sym]) & 0xFFFF)
    assert t.huff.shape == (4, 256) and t.huff.dtype == np.uint32
    assert entry(0, 0) == (2, 0b00) and entry(0, 11) == (9, 0b111111110)                 # table K.3
    assert entry(1, 0x00) == (4, 0b1010) and entry(1, 0xF0) == (11, 0b11111111001) and entry(1, 0x01) == (2, 0b00)      # table K.5
    assert entry(2, 0) == (2, 0b00) and entry(2, 11) == (11, 0b11111111110)              # table K.4
    assert entry(3, 0x00) == (2, 0b00) and entry(3, 0xF0) == (10, 0b1111111010) and entry(3, 0xFA) == (16, 0xFFFE)      # table K.6
    for tab in range(4):                                                         # prefix-free: Kraft sum of a full-but-one code
        lengths = (t.huff[tab] >> 16)[t.huff[tab] >> 16 > 0].astype(np.int64)
        assert len(lengths) == (12, 162, 12, 162)[tab] and sum(2.0 ** -lengths) < 1.0
    assert entry(1, 0x0B) == (0, 0)                                              # AC category 11 has no code
    with pytest.raises(ValueError, match="BITS"):
        V.huffman_codes((1,) + (0,) * 15, b"\x00\x01")


def test_quality_scaling_is_the_ijg_rule():
    assert int(V.jpeg_tables(50).quant[0, 0]) == 16 and int(V.jpeg_tables(50).quant[1, 63]) == 99
    assert np.all(V.jpeg_tables(100).quant == 1)
    assert int(V.jpeg_tables(1).quant[0, 0]) == 255 and int(V.jpeg_tables(1).quant.min()) == 255      # 16 * 5000 / 100, clamped
    assert int(V.jpeg_tables(25).quant[0, 0]) == 32 and int(V.jpeg_tables(75).quant[0, 0]) == 8
    for bad in (0, 101, -5, 90.0, True, None):
        with pytest.raises(ValueError, match="1 to 100"):
            V.jpeg_tables(bad)


# ------------------------------------------------------------------------------------------------------------------------------ framing
def test_finish_scan_pads_with_ones_and_stuffs_zero_after_ff():
    assert V.finish_scan(np.array([0xAB, 0xC0, 0x00], np.uint8), 10) == bytes([0xAB, 0xFF, 0x00]) + b"\xFF\xD9"     # 6 pad bits, then stuffed
    assert V.finish_scan(np.array([0xFF, 0xFF, 0x12], np.uint8), 24) == bytes([0xFF, 0, 0xFF, 0, 0x12]) + b"\xFF\xD9"
    assert V.finish_scan(np.array([0x80, 0x55], np.uint8), 1) == bytes([0xFF, 0x00]) + b"\xFF\xD9"                  # bytes behind the stream are not read
    assert V.finish_scan(np.zeros(4, np.uint8), 16) == b"\x00\x00\xFF\xD9"
    src = np.array([1, 2, 3], np.uint8)
    V.finish_scan(src, 17)
    assert src.tolist() == [1, 2, 3]                                             # the caller's buffer is left alone


@pytest.mark.parametrize("quality", R.QUALITIES)
@pytest.mark.parametrize("content", R.CONTENTS)
def test_pillow_decodes_the_framed_reference_streams(content, quality):
    t = V.jpeg_tables(quality)
    for n, H, W in R.SHAPES:
        frames = R.make_frames(content, n, H, W)
        coefs, _ = R.blocks(frames, t.quant)
        mr, mc = R.n_mcus(H, W)
        assert coefs.shape == (n, mr * mc, 6, 64)
        counts, streams, _ = R.entropy(coefs, t.huff)
        for i, (stream, bits) in enumerate(streams):
            assert bits == int(counts[i].sum()) and len(stream) == (bits + 7) // 8
            jpeg = V.jpeg_header(H, W, quality) + V.finish_scan(stream, bits)
            check_decodes_within_gate(jpeg, frames[i], quality, DEFICIT_DB[content, quality] + GATE_MARGIN_DB, f"{content} q{quality} {H}x{W} #{i}")


def test_the_shared_frames_reach_the_corners_of_the_code():
    seen = {}
    for content, quality in (("flat", 90), ("noise", 100), ("impulses", 50), ("impulses", 10)):
        t = V.jpeg_tables(quality)
        tot = dict(dc_category=0, ac_category=0, zrl=0, ff=0, nonzero_ac=0, dc_diffs=0)
        for n, H, W in R.SHAPES:
            coefs, _ = R.blocks(R.make_frames(content, n, H, W), t.quant)
            _, streams, s = R.entropy(coefs, t.huff)
            tot["dc_category"], tot["ac_category"] = max(tot["dc_category"], s["dc_category"]), max(tot["ac_category"], s["ac_category"])
            tot["zrl"] += s["zrl"]
            tot["ff"] += sum(int((st == 0xFF).sum()) for st, _ in streams)
            tot["nonzero_ac"] += int((coefs[..., 1:] != 0).sum())
            flat_mcus = coefs[:, 1:, :, 0] - coefs[:, :1, :, 0]
            tot["dc_diffs"] += int((flat_mcus != 0).sum())
        seen[content, quality] = tot
    assert seen["flat", 90]["nonzero_ac"] == 0 and seen["flat", 90]["dc_diffs"] == 0      # EOB-only blocks, zero DC differences
    assert seen["noise", 100]["dc_category"] == 11 and seen["noise", 100]["ac_category"] == 10 and seen["noise", 100]["ff"] > 0
    assert seen["impulses", 50]["zrl"] > 0
    assert seen["impulses", 10]["zrl"] == 0            # (the header's reasoning)


# ------------------------------------------------------------------------------------------------------------------------------ AVI
def fake_jpegs(n, seed=0):
    rng = np.random.default_rng(seed)
    sizes = [101, 100, 57, 1, 2, 255][:n] + [int(s) for s in rng.integers(20, 300, max(0, n - 6))]
    return [bytes(rng.integers(0, 256, s, dtype=np.uint8)) for s in sizes]


def riff_tree(raw, pos, end):
    out = []
    while pos < end:
        cid, size = raw[pos:pos + 4], struct.unpack_from("<I", raw, pos + 4)[0]
        assert pos + 8 + size <= end, (cid, pos, size, end)
        if size & 1:
            assert raw[pos + 8 + size] == 0                                      # the pad byte of an odd-sized chunk
        out.append((cid, pos, size))
        pos += 8 + size + (size & 1)
    assert pos == end
    return out


def check_avi_structure(raw, n_frames, n_audio_chunks):
    assert raw[:4] == b"RIFF" and raw[8:12] == b"AVI " and struct.unpack_from("<I", raw, 4)[0] == len(raw) - 8
    top = riff_tree(raw, 12, len(raw))
    assert [(c, raw[p + 8:p + 12] if c == b"LIST" else None) for c, p, _ in top] == [(b"LIST", b"hdrl"), (b"LIST", b"movi"), (b"idx1", None)]
    (_, hdrl, hdrl_size), (_, movi, movi_size), (_, idx, idx_size) = top
    assert [c for c, _, _ in riff_tree(raw, hdrl + 12, hdrl + 8 + hdrl_size)] == [b"avih"] + [b"LIST"] * (2 if n_audio_chunks else 1)
    chunks = riff_tree(raw, movi + 12, movi + 8 + movi_size)
    assert [c for c, _, _ in chunks].count(b"00dc") == n_frames and [c for c, _, _ in chunks].count(b"01wb") == n_audio_chunks
    assert idx_size == 16 * len(chunks)
    for k, (cid, pos, size) in enumerate(chunks):                                # idx1: the chunk's id, key-frame flag, offset from `movi`, size
        assert struct.unpack_from("<4sIII", raw, idx + 8 + 16 * k) == (cid, 0x10, pos - (movi + 8), size)
    assert struct.unpack_from("<I", raw, hdrl + 12 + 8 + 16)[0] == n_frames      # avih.dwTotalFrames
    return chunks


@pytest.mark.parametrize("fps,want", [(25, Fraction(25)), (Fraction(30000, 1001), Fraction(30000, 1001)), (8, Fraction(8)),
                                      ((30000, 1001), Fraction(30000, 1001))])
def test_avi_round_trip(tmp_path, fps, want):
    jpegs = fake_jpegs(9, 1)
    path = tmp_path / "clip.avi"
    V.write_avi(path, jpegs, 38, 70, fps)
    got, got_fps, audio = V.read_avi(path)
    assert got == jpegs and got_fps == want and audio is None
    raw = path.read_bytes()
    check_avi_structure(raw, 9, 0)
    assert raw.count(b"vidsMJPG") == 1 and struct.unpack_from("<II", raw, raw.index(b"vidsMJPG") + 20) == (want.denominator, want.numerator)
    strf = raw.index(b"strf") + 8
    assert struct.unpack_from("<IiiHH4s", raw, strf) == (40, 38, 70, 1, 24, b"MJPG")


@pytest.mark.parametrize("fps", [25, Fraction(30000, 1001), 8])
@pytest.mark.parametrize("channels", [1, 2])
def test_avi_audio_round_trip_loses_and_repeats_no_sample(tmp_path, fps, channels):
    n_frames, rate = 11, 16000
    f = Fraction(fps)
    n = int(n_frames * rate / f) + 3                                             # a little more than the clip: the rest rides with the last frame
    rng = np.random.default_rng(5)
    x = rng.uniform(-1.2, 1.2, (n, channels)).astype(np.float32)                 # some samples clip
    x[:4, 0] = (1.0, -1.0, 0.5 / 32767, 1.5 / 32767)
    want = np.rint(np.clip(x.astype(np.float64), -1, 1) * 32767).astype(np.int16)
    assert want[:2, 0].tolist() == [32767, -32767] and int(want.max()) == 32767 and int(want.min()) == -32767
    path = tmp_path / "clip.avi"
    jpegs = fake_jpegs(n_frames, 2)
    V.write_avi(path, jpegs, 16, 16, fps, audio=(x if channels == 2 else x[:, 0], rate))
    got, got_fps, (pcm, got_rate) = V.read_avi(path)
    assert got == jpegs and got_fps == f and got_rate == rate
    assert pcm.dtype == np.int16 and pcm.shape == want.shape and np.array_equal(pcm, want)
    raw = path.read_bytes()
    chunks = check_avi_structure(raw, n_frames, n_frames)
    assert [c for c, _, _ in chunks] == [b"00dc", b"01wb"] * n_frames            # interleaved per frame
    sizes = [s // (2 * channels) for c, _, s in chunks if c == b"01wb"]
    cuts = [int(i * rate / f + Fraction(1, 2)) for i in range(n_frames)] + [n]   # cumulative rounding
    assert sizes == [b - a for a, b in zip(cuts, cuts[1:])] and sum(sizes) == n
    if f.denominator != 1:
        assert len(set(sizes[:-1])) > 1                                          # 16000 * 1001 / 30000 = 533.87: the chunks differ
    fmt = raw.index(b"auds")
    assert struct.unpack_from("<HHIIHHH", raw, raw.index(b"strf", fmt) + 8) == (1, channels, rate, rate * 2 * channels, 2 * channels, 16, 0)


def test_avi_audio_shorter_than_the_clip_and_torch_samples(tmp_path):
    path = tmp_path / "short.avi"
    x = torch.linspace(-1, 1, 1000)
    V.write_avi(path, fake_jpegs(6, 3), 8, 8, 25, audio=(x, 8000))             # 320 samples per frame: the audio ends inside frame 3
    _, _, (pcm, rate) = V.read_avi(path)
    assert rate == 8000 and np.array_equal(pcm[:, 0], np.rint(x.double().numpy() * 32767).astype(np.int16))
    chunks = check_avi_structure(path.read_bytes(), 6, 4)
    assert [s for c, _, s in chunks if c == b"01wb"] == [640, 640, 640, 80]


def test_read_avi_refuses_what_write_avi_did_not_make(tmp_path):
    path = tmp_path / "a.avi"
    V.write_avi(path, fake_jpegs(3), 8, 8, 25)
    raw = path.read_bytes()
    for name, data in (("truncated", raw[:-5]), ("wave", raw[:8] + b"WAVE" + raw[12:]), ("codec", raw.replace(b"vidsMJPG", b"vidsH264")),
                       ("junk", raw + b"JUNK\x00\x00\x00\x00"), ("empty", b"")):
        p = tmp_path / f"{name}.avi"
        p.write_bytes(data)
        with pytest.raises(ValueError, match="read_avi"):
            V.read_avi(p)


# ------------------------------------------------------------------------------------------------------------------------------ the grid
def grid_by_hand(videos, n_rows, rescale):
    """torchvision.utils.make_grid(x, nrow=n_rows) (padding 2, pad value 0) per time step, pixel by pixel"""
    b, c, t, h, w = videos.shape
    v = videos.numpy().astype(np.float32)
    if b == 1:
        out = v[0].transpose(1, 2, 3, 0)
    else:
        xmaps = min(n_rows, b)
        ymaps = -(-b // xmaps)
        out = np.zeros((t, (h + 2) * ymaps + 2, (w + 2) * xmaps + 2, 3), np.float32)
        for k in range(b):
            y0, x0 = (k // xmaps) * (h + 2) + 2, (k % xmaps) * (w + 2) + 2
            out[:, y0:y0 + h, x0:x0 + w] = v[k].transpose(1, 2, 3, 0)
    if rescale:                                                                  # util.py:28 follows make_grid: the border turns mid-grey
        out = (out + np.float32(1.0)) / np.float32(2.0)
    return (out * np.float32(255)).astype(np.uint8)


@pytest.mark.parametrize("b,n_rows,size", [(1, 6, (5, 7)), (3, 2, (2 * 7 + 2, 2 * 9 + 2)), (7, 6, (2 * 7 + 2, 6 * 9 + 2))])
def test_save_videos_grid_geometry(b, n_rows, size):
    g = torch.Generator().manual_seed(b)
    videos = torch.rand(b, 3, 4, 5, 7, generator=g)
    got = V.make_grid_u8(videos, n_rows=n_rows)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (4, *size, 3) and got.is_contiguous()
    assert np.array_equal(got.numpy(), grid_by_hand(videos, n_rows, False))
    if b > 1:
        assert int(got[:, :2].max()) == 0 and int(got[:, :, :2].max()) == 0 and int(got[:, 7:9].max()) == 0      # the borders
        assert np.array_equal(got[:, 2:7, 2:9].numpy(), (videos[0] * 255).to(torch.uint8).permute(1, 2, 3, 0).numpy())
    if b == 7:
        assert int(got[:, 9:, 11:].max()) == 0                                   # the six empty cells of the second row
        assert int(got[:, 9:14, 2:9].max()) > 0                                  # image 6 sits at (1 * 7 + 2, 2)
    signed = videos * 2 - 1
    assert np.array_equal(V.make_grid_u8(signed, rescale=True, n_rows=n_rows).numpy(), grid_by_hand(signed, n_rows, True))
    one = V.make_grid_u8(videos[:, :1], n_rows=n_rows)                           # a single channel is repeated
    assert torch.equal(one[..., 0], one[..., 1]) and torch.equal(one[..., 0], one[..., 2]) and tuple(one.shape) == tuple(got.shape)


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_only_avi_is_written(tmp_path):
    videos = torch.rand(1, 3, 2, 8, 8)
    for name in ("clip.mp4", "clip.gif", "clip", "clip.avi.mp4"):
        with pytest.raises(ValueError, match=r"\.avi"):
            V.save_videos_grid(videos, str(tmp_path / name))
        with pytest.raises(ValueError, match=r"\.avi"):
            V.images2video([np.zeros((8, 8, 3), np.uint8)], str(tmp_path / name))
        with pytest.raises(ValueError, match=r"\.avi"):
            V.write_video(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), tmp_path / name, 25)
    assert list(tmp_path.iterdir()) == []


def test_write_avi_refuses_two_gib_and_bad_arguments(tmp_path):
    blob = bytes(1 << 20)
    path = tmp_path / "big.avi"
    with pytest.raises(ValueError, match="OpenDML"):
        V.write_avi(path, [blob] * 2048, 16, 16, 25)                             # 2^31 bytes of frames alone
    V.write_avi(path, [blob] * 3, 16, 16, 25)                                    # (the same blob is fine in a file that fits)
    assert len(V.read_avi(path)[0]) == 3
    os.remove(path)
    with pytest.raises(ValueError, match="OpenDML"):
        V.write_avi(path, [blob] * 2047, 16, 16, 25, audio=(np.zeros(1 << 20, np.float32), 16000))       # the audio tips it over
    assert not path.exists()
    for bad in (0, -3, 2.5, "25", (25,), (0, 1), True):
        with pytest.raises(ValueError, match="fps"):
            V.write_avi(path, [b"x"], 16, 16, bad)
    with pytest.raises(ValueError, match="frames"):
        V.write_avi(path, [], 16, 16, 25)
    with pytest.raises(ValueError, match="samples"):
        V.write_avi(path, [b"x"], 16, 16, 25, audio=(np.zeros((2, 2, 2)), 16000))


def test_encode_mjpeg_refuses_bad_quality_and_frames():
    frames = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    for bad in (0, 101):
        with pytest.raises(ValueError, match="1 to 100"):
            V.encode_mjpeg(frames, quality=bad)
    for bad in (frames.float(), torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 8, 4, dtype=torch.uint8), np.zeros((1, 8, 8, 3), np.uint8)):
        with pytest.raises(ValueError, match="uint8 RGB frames"):
            V.encode_mjpeg(bad)


def test_call_save_path_refusals(tmp_path):
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    p = EMOAnimationPipeline(unet=SimpleNamespace(device=torch.device("cpu")), scheduler=DDIMScheduler())      # no VAE
    good = str(tmp_path / "clip.avi")
    with pytest.raises(ValueError, match=r"\.avi"):
        p("", 2, save_path=str(tmp_path / "clip.mp4"), fps=25)
    with pytest.raises(ValueError, match="fps="):
        p("", 2, save_path=good)
    with pytest.raises(ValueError, match="VAE"):
        p("", 2, save_path=good, fps=25)
    for bad in (0, 101):
        with pytest.raises(ValueError, match="1 to 100"):
            p("", 2, save_path=good, fps=25, save_quality=bad)
    assert list(tmp_path.iterdir()) == []


def test_audio_for_file_takes_paths_and_pairs(tmp_path):
    from emote_hack_amd.pipeline import EMOAnimationPipeline as P
    x = np.linspace(-0.5, 0.5, 40, dtype=np.float32).reshape(20, 2)
    samples, rate = P._audio_for_file((x, 44100))
    assert rate == 44100 and samples.shape == (20, 2) and np.array_equal(samples, x)
    samples, rate = P._audio_for_file((torch.from_numpy(x[:, 0].copy()), 8000))
    assert rate == 8000 and samples.shape == (20, 1)
    wav = tmp_path / "a.wav"
    pcm = np.rint(x * 32767).astype("<i2")
    wav.write_bytes(b"RIFF" + struct.pack("<I", 36 + pcm.nbytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 2, 22050, 22050 * 4, 4, 16)
                    + b"data" + struct.pack("<I", pcm.nbytes) + pcm.tobytes())
    samples, rate = P._audio_for_file(str(wav))
    assert rate == 22050 and samples.shape == (20, 2) and np.array_equal(V.pcm16(samples * (32768 / 32767)), pcm)
    assert P._audio_for_file(torch.zeros(100)) is None and P._audio_for_file(None) is None and P._audio_for_file("clip.mp4") is None
