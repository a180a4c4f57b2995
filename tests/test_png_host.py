"""Host tests of the PNG / APNG writer (no GPU): the serial reference of tests/png_ref.py makes streams zlib inflates and files Pillow
opens; the Huffman builder, the block header, the Adler-32 combination, the containers and the refusals of emote_hack_amd.video_io."""
import heapq
import io
import struct
import zlib
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from emote_hack_amd import video_io as V
from tests import gif_ref
from tests import png_ref as R


def images():
    rng = np.random.default_rng(3)
    flat = np.full((1, 9, 40, 3), 77, np.uint8)
    return {"noisy_rgb": gif_ref.synthetic_clip(1, 21, 19, 4), "portrait": R.synthetic_portrait(2, 24, 31, 1), "flat": flat,
            "grey": rng.integers(0, 256, (1, 7, 13, 1), dtype=np.uint8), "rgba": gif_ref.synthetic_clip(1, 6, 5, 2).repeat(2, axis=3)[..., :4].copy(),
            "pixel": np.array([[[[200]]]], np.uint8), "random": rng.integers(0, 256, (1, 5, 11, 3), dtype=np.uint8)}


@pytest.mark.parametrize("name", sorted(images()))
@pytest.mark.parametrize("strip_rows", [1, 8, None])
def test_reference_streams_inflate_and_pillow_opens_the_files(name, strip_rows):
    frames = images()[name]
    n, H, W, C = frames.shape
    filtered, files = R.reference_files(frames, 5, strip_rows, V.deflate_tables)
    for f in range(n):
        chunks = R.parse_chunks(files[f])
        assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
        stream = chunks[1][1]
        assert R.first_block_type(stream) == (1, 2)                              # one final block, dynamic Huffman codes
        assert zlib.decompress(stream) == filtered[f].tobytes()                  # inflate checks the Adler-32 too
        assert files[f] == V.png_container(W, H, C, stream)
        got = np.asarray(Image.open(io.BytesIO(files[f])))
        assert np.array_equal(got.reshape(H, W, C), frames[f]), (name, f)


@pytest.mark.parametrize("filter", [0, 1, 2, 3, 4])
def test_forced_filters_decode(filter):
    frames = images()["noisy_rgb"]
    filtered, files = R.reference_files(frames, filter, 4, V.deflate_tables)
    assert (filtered[:, :, 0] == filter).all()
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[0]))), frames[0])


def test_host_places_header_end_of_block_and_checksum():
    """zlib_stream turns what the emit kernel leaves - the tokens alone, at their bits - into the reference's stream"""
    frames = images()["portrait"]
    filtered = R.filter_frames(frames, 5)
    for f in range(2):
        _, hist = R.tokenize_frame(filtered[f], 8)
        t = V.deflate_tables(hist)
        want = R.zlib_stream(filtered[f], 8, t)
        token_bits = t.token_bits(hist)
        code, length = t.end_of_block
        assert len(want) == (16 + t.header_bits + token_bits + length + 7) // 8 + 4
        host_part = np.zeros(len(want), np.uint8)                                # everything the host adds, to take it out of the stream
        host_part[:2] = 0xFF
        V._or_bits(host_part, 16, (1 << t.header_bits) - 1, t.header_bits)
        V._or_bits(host_part, 16 + t.header_bits + token_bits, (1 << length) - 1, length)
        host_part[-4:] = 0xFF
        tokens_only = np.frombuffer(want, np.uint8) & ~host_part
        adler = V.adler32_combine(R.adler_pairs(filtered[f]), filtered.shape[-1])
        assert adler == zlib.adler32(filtered[f].tobytes())
        assert V.zlib_stream(tokens_only, t, token_bits, adler) == want
        with pytest.raises(ValueError, match="bytes for a block"):
            V.zlib_stream(tokens_only[:-1], t, token_bits, adler)


# ------------------------------------------------------------------------------------------------------------------------------ Huffman
def kraft(lengths):
    return sum(Fraction(1, 2 ** l) for l in lengths if l)


def plain_huffman(freq):
    """-> (total bits, depth of the deepest leaf) of a plain Huffman tree"""
    heap = [(f, i, 0) for i, f in enumerate(freq) if f > 0]
    heapq.heapify(heap)
    total = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        total += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), max(a[2], b[2]) + 1))
    return total, heap[0][2]


def plain_huffman_bits(freq):
    return plain_huffman(freq)[0]


def test_huffman_lengths_are_complete_and_limited():
    rng = np.random.default_rng(0)
    for trial in range(20):
        freq = rng.integers(20, 1000, 286) * (rng.random(286) < 0.6)
        freq[256] = 20
        bits, depth = plain_huffman(freq)
        assert depth <= 15                                                       # the unlimited lengths fit: the builder gives the minimum
        lengths = V.huffman_code_lengths(freq, 15)
        assert all((l > 0) == (f > 0) for l, f in zip(lengths, freq)) and max(lengths) <= 15 and kraft(lengths) == 1
        assert sum(int(f) * l for f, l in zip(freq, lengths)) == bits
    for trial in range(5):                                                       # rare symbols beside common ones: the limit binds or not, complete either way
        freq = rng.integers(0, 1000, 286) * (rng.random(286) < 0.6)
        freq[256] = 1
        lengths = V.huffman_code_lengths(freq, 15)
        assert all((l > 0) == (f > 0) for l, f in zip(lengths, freq)) and max(lengths) <= 15 and kraft(lengths) == 1
        assert sum(int(f) * l for f, l in zip(freq, lengths)) >= plain_huffman_bits(freq)
    for n in (2, 3, 19):
        lengths = V.huffman_code_lengths([1] * n, 7)
        assert kraft(lengths) == 1 and max(lengths) <= 7


def test_huffman_limiter():
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    for limit, freq in ((15, fib), (7, fib[:19]), (15, fib + [0] * 200 + fib)):
        used = [f for f in freq if f]
        assert plain_huffman_bits(freq) < sum(used) * 40
        lengths = V.huffman_code_lengths(freq, limit)
        assert max(lengths) == limit and kraft(lengths) == 1 and all((l > 0) == (f > 0) for l, f in zip(lengths, freq))
        assert sum(f * l for f, l in zip(freq, lengths)) > plain_huffman_bits(freq)      # the plain tree is deeper than the limit
        order = sorted(range(len(freq)), key=lambda i: freq[i])
        assert all(lengths[a] >= lengths[b] for a, b in zip(order, order[1:]) if freq[a] and freq[a] < freq[b])      # rarer symbols: longer codes
    with pytest.raises(ValueError, match="do not fit"):
        V.huffman_code_lengths([1] * 9, 3)


def test_huffman_edge_rules_of_the_distance_alphabet():
    assert V.huffman_code_lengths([0] * 30, 15) == [0] * 30
    one = V.huffman_code_lengths([0] * 7 + [9] + [0] * 22, 15)
    assert one[7] == 1 and sum(one) == 1
    assert kraft(V.huffman_code_lengths([0, 0, 5, 0], 7, complete=True)) == 1      # the code-length code is always complete
    hist = np.zeros(320, np.int64)
    hist[[0, 65, 66, 256]] = [3, 5, 2, 1]
    t = V.deflate_tables(hist)                                                   # no distance symbol: HDIST = 0, one code of length 0
    assert not t.lengths[288:].any() and (t.header >> 8) & 31 == 0
    hist[257], hist[288] = 4, 4
    t = V.deflate_tables(hist)                                                   # exactly one: length 1
    assert t.lengths[288] == 1 and not t.lengths[289:].any()
    for bad in (np.zeros(320, np.int64), np.zeros(319, np.int64), np.zeros(320)):
        with pytest.raises(ValueError):
            V.deflate_tables(bad)


def test_canonical_codes_and_the_table_layout():
    assert V.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15]      # the example of RFC 1951 3.2.2
    assert V.canonical_codes([2, 1, 3, 3]) == R.canonical([2, 1, 3, 3])
    hist = R.tokenize_frame(R.filter_frames(images()["portrait"], 5)[0], 8)[1]
    t = V.deflate_tables(hist)
    assert t.lengths.max() <= 15 and (t.codes >> 16 == t.lengths).all() and ((t.lengths > 0) == (hist > 0)).all()
    lit = R.canonical([int(l) for l in t.lengths[:286]])
    for sym in np.flatnonzero(hist[:286]):
        n = int(t.lengths[sym])
        assert int(t.codes[sym] & 0xFFFF) == int(format(lit[sym], f"0{n}b")[::-1], 2)
    assert t.header & 7 == 0b101                                                 # BFINAL = 1, BTYPE = 2


def test_length_runs():
    runs = V.deflate_length_runs([0] * 150 + [5] * 9 + [0, 0] + [3] + [0] * 7 + [4, 4, 4])
    assert runs == [(18, 7, 127), (18, 7, 1), (5, 0, 0), (16, 2, 3), (5, 0, 0), (5, 0, 0), (0, 0, 0), (0, 0, 0), (3, 0, 0), (17, 3, 4),
                    (4, 0, 0), (4, 0, 0), (4, 0, 0)]


def test_adler32_combine():
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes() + b"\xff" * 9000
    for cuts in ([1, 2, 3, 70000, 70001], [5551, 5553, 11111, 65521, 65522], [39999], []):
        pieces = [data[a:b] for a, b in zip([0] + cuts, cuts + [len(data)])]
        pairs = [(zlib.adler32(p) & 0xFFFF, zlib.adler32(p) >> 16) for p in pieces]
        assert V.adler32_combine(pairs, [len(p) for p in pieces]) == zlib.adler32(data), cuts
    rows = np.frombuffer(data[:78000], np.uint8).reshape(-1, 13)
    assert V.adler32_combine(R.adler_pairs(rows[None])[0], 13) == zlib.adler32(rows.tobytes())


# ------------------------------------------------------------------------------------------------------------------------------ containers
@pytest.mark.parametrize("fps, delay", [(25, (1, 25)), (Fraction(30000, 1001), (1001, 30000)), ((30000, 1001), (1001, 30000)), (8, (1, 8))])
def test_apng_chunks(fps, delay):
    streams = [zlib.compress(bytes([0, i, i, i]) * 2) for i in range(3)]
    data = V.apng_container(1, 2, 3, streams, fps, loop=4)
    chunks = R.parse_chunks(data)
    assert [k for k, _ in chunks] == [b"IHDR", b"acTL", b"fcTL", b"IDAT", b"fcTL", b"fdAT", b"fcTL", b"fdAT", b"IEND"]
    assert struct.unpack(">II", chunks[1][1]) == (3, 4)
    seq = []
    for kind, body in chunks:
        if kind == b"fcTL":
            s, w, h, x, y, num, den, dispose, blend = struct.unpack(">IIIIIHHBB", body)
            assert (w, h, x, y, num, den, dispose, blend) == (1, 2, 0, 0) + delay + (0, 0)
            seq.append(s)
        elif kind == b"fdAT":
            seq.append(struct.unpack(">I", body[:4])[0])
            assert body[4:] in streams[1:]
    assert seq == [0, 1, 2, 3, 4] and chunks[3][1] == streams[0]
    im = Image.open(io.BytesIO(data))
    assert im.n_frames == 3 and im.info["loop"] == 4
    assert im.info["duration"] == pytest.approx(1000 * delay[0] / delay[1])


def test_apng_refusals():
    stream = [zlib.compress(b"\0\0")]
    for fps in (65536, Fraction(1, 65536), Fraction(65537, 65536), (70001, 70000)):
        with pytest.raises(ValueError, match="65535"):
            V.apng_container(1, 1, 1, stream, fps)
        with pytest.raises(ValueError, match="65535"):
            V.encode_apng(torch.zeros(1, 2, 2, 3, dtype=torch.uint8), fps)
    with pytest.raises(ValueError, match="loop="):
        V.apng_container(1, 1, 1, stream, 25, loop=-1)
    with pytest.raises(ValueError, match="no frames"):
        V.apng_container(1, 1, 1, [], 25)
    with pytest.raises(ValueError, match="channels"):
        V.apng_container(1, 1, 2, stream, 25)
    assert V.apng_delay(Fraction(65535, 65534)) == (65534, 65535)


def test_arguments_are_checked_before_any_launch(tmp_path):
    """host tensors: a launch would raise EmoHipError, so every ValueError here was raised before one"""
    frames = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    for bad in (frames.float(), torch.zeros(8, 8, dtype=torch.uint8), torch.zeros(1, 8, 8, 2, dtype=torch.uint8), np.zeros((1, 8, 8, 3), np.uint8)):
        with pytest.raises(ValueError, match="uint8 frames"):
            V.encode_png(bad)
    with pytest.raises(ValueError, match="no frames"):
        V.encode_png(torch.zeros(0, 8, 8, 3, dtype=torch.uint8))
    for kw, match in ((dict(filter="best"), "filter="), (dict(filter=5), "filter="), (dict(strip_rows=0), "strip_rows="),
                      (dict(strip_rows=2.5), "strip_rows="), (dict(strip_rows=True), "strip_rows=")):
        with pytest.raises(ValueError, match=match):
            V.encode_png(frames, **kw)
        with pytest.raises(ValueError, match=match):
            V.encode_apng(frames, 25, **kw)
        with pytest.raises(ValueError, match=match):
            V.write_video(frames, tmp_path / "clip.apng", 25, format="apng", **kw)
    with pytest.raises(ValueError, match="65535 bytes of a strip"):
        V.encode_png(torch.zeros(1, 1, 21845, 3, dtype=torch.uint8))             # 1 + 3 * 21845 = 65536 bytes in one scanline
    assert V.png_strip_rows(8, 512, 512, 3) == 8 and V.png_strip_rows(None, 512, 512, 3) == 42 and V.png_strip_rows(8, 5, 9, 1) == 5
    assert V.png_strip_rows(8, 100, 21844, 3) == 1 and V.png_strip_rows(3, 100, 5000, 4) == 3 and V.png_strip_rows(4, 100, 5000, 4) == 3
    assert list(tmp_path.iterdir()) == []


def test_write_png_patterns(tmp_path):
    one, two = torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(2, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"%04d.*\.apng"):
        V.write_png(two, tmp_path / "frame.png")                                 # several frames, one name: both ways out are named
    for name in ("frame.jpg", "frame", "frame.apng", "frame_%04d.gif"):
        with pytest.raises(ValueError, match=r"\.png"):
            V.write_png(one, tmp_path / name)
    for name in ("f_%d_%d.png", "f_%s.png", "f_%5.2f.png", "f_%.png"):
        with pytest.raises(ValueError, match="one field"):
            V.write_png(two, tmp_path / name)
    with pytest.raises(ValueError, match="one field"):
        V.write_png(two, tmp_path / "d_%d" / "f.png")
    assert V._png_pattern("a/f_%04d.png", "w") == ("a/f_%04d.png", True) and V._png_pattern("f%d.PNG", "w")[1] and not V._png_pattern("f.png", "w")[1]
    assert V._png_pattern("100%%_%03d.png", "w")[1]
    assert list(tmp_path.iterdir()) == []


def test_reference_surface_refusals(tmp_path):
    frames = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    videos, stills = torch.rand(1, 3, 2, 8, 8), [np.zeros((8, 8, 3), np.uint8)]
    good = str(tmp_path / "clip.apng")
    for name in ("clip.avi", "clip.png", "clip.gif", "clip"):
        with pytest.raises(ValueError, match=r"\.apng"):
            V.write_video(frames, tmp_path / name, 25, format="apng")
        with pytest.raises(ValueError, match=r"\.apng"):
            V.save_videos_grid(videos, str(tmp_path / name), format="apng")
        with pytest.raises(ValueError, match=r"\.apng"):
            V.images2video(stills, str(tmp_path / name), format="apng")
    for kw in (dict(quality=50), dict(restart_interval="row")):
        with pytest.raises(ValueError, match="quality= and restart_interval="):
            V.write_video(frames, good, 25, format="apng", **kw)
        with pytest.raises(ValueError, match="quality= and restart_interval="):
            V.save_videos_grid(videos, good, format="apng", **kw)
        with pytest.raises(ValueError, match="quality= and restart_interval="):
            V.images2video(stills, good, format="apng", **kw)
    with pytest.raises(ValueError, match="audio="):
        V.write_video(frames, good, 25, format="apng", audio=(np.zeros(100, np.float32), 16000))
    with pytest.raises(ValueError, match="unknown option"):
        V.write_video(frames, good, 25, format="apng", colors=16)
    with pytest.raises(ValueError, match="format=\"apng\""):
        V.write_video(frames, tmp_path / "clip.avi", 25, filter="paeth")
    with pytest.raises(ValueError, match="unknown option"):
        V.write_apng(frames, good, 25, quality=90)
    for name in ("grid.gif", "grid.avi", "grid"):
        with pytest.raises(ValueError, match=r"`\.png`.*`\.jpg`"):
            V.save_images_grid(torch.rand(2, 3, 1, 4, 4), str(tmp_path / name))
    with pytest.raises(ValueError, match="b, c, 1, h, w"):
        V.save_images_grid(torch.rand(2, 3, 2, 4, 4), str(tmp_path / "grid.png"))
    assert list(tmp_path.iterdir()) == []


def test_call_save_path_png_refusals(tmp_path):
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    p = EMOAnimationPipeline(unet=SimpleNamespace(device=torch.device("cpu")), scheduler=DDIMScheduler())      # no VAE
    clip, stills = str(tmp_path / "clip.apng"), str(tmp_path / "f_%04d.png")
    with pytest.raises(ValueError, match="fps="):
        p("", 2, save_path=clip)
    with pytest.raises(ValueError, match="VAE"):
        p("", 2, save_path=clip, fps=8)                                          # an `.apng` path is taken; the checks go on to the next one
    with pytest.raises(ValueError, match="VAE"):
        p("", 2, save_path=stills)                                               # numbered stills need no fps=
    with pytest.raises(ValueError, match=r"%04d.*\.apng"):
        p("", 2, save_path=str(tmp_path / "clip.png"))
    with pytest.raises(ValueError, match="VAE"):
        p("", 1, save_path=str(tmp_path / "clip.png"))                           # one frame, one name
    for path in (clip, stills):
        for kw, match in ((dict(save_restart_interval="row"), "save_restart_interval="), (dict(save_quality=50), "save_quality="),
                          (dict(save_palette="frame"), "save_palette="), (dict(save_dither="bayer"), "save_dither="),
                          (dict(save_png_filter="best"), "filter=")):
            with pytest.raises(ValueError, match=match):
                p("", 2, save_path=path, fps=8, **kw)
    with pytest.raises(ValueError, match="save_loop="):
        p("", 2, save_path=clip, fps=8, save_loop=-1)
    with pytest.raises(ValueError, match="save_loop="):
        p("", 2, save_path=stills, save_loop=1)
    with pytest.raises(ValueError, match="65535"):
        p("", 2, save_path=clip, fps=Fraction(65537, 2))
    with pytest.raises(ValueError, match="65535"):
        p("", 2, save_path=clip, fps=40000, interpolation_factor=2)              # the file plays at fps * interpolation_factor
    assert list(tmp_path.iterdir()) == []


def test_lazy_exports():
    import emote_hack_amd
    for name in ("save_images_grid", "encode_png", "encode_apng", "write_png", "write_apng"):
        assert getattr(emote_hack_amd, name) is getattr(V, name)
