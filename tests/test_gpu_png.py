"""GPU tests of the PNG / APNG writer: emo_png_filter / emo_png_lz_count / emo_png_deflate_bits / emo_png_deflate_emit (csrc/png_out.hip)
against tests/png_ref.py, and the files of encode_png, encode_apng, the reference surface and `__call__(save_path=...)` through zlib's
inflate and Pillow's decoder.  Everything is exact: the filtered bytes, the tokens, the histograms and the files equal the serial
reference's byte for byte, and a decoded file equals the frames byte for byte.

The shapes are the smallest that reach each way the kernels can go: odd sizes with tail lanes and several strips (2x37x53xC), one pixel,
one column, rows built so that every filter type wins the adaptive choice, flat frames (the longest matches, capped at the strip's end),
repeated rows (a distance of one row), strips of one row, of 8 and of the whole frame, a short last strip, two triples in one hash slot,
a strip near the 65535-byte limit (the kernel's large-LDS launch), and frames whose streams end at different bit phases."""
import ctypes
import functools
import io
import zlib
from fractions import Fraction

import numpy as np
import pytest
import torch
from PIL import Image

from emote_hack_amd import _lib
from emote_hack_amd import video_io as V
from emote_hack_amd._lib import EmoHipError
from tests import gif_ref
from tests import png_ref as R
from tests.test_gpu_kernels import DEV, ops

pytestmark = pytest.mark.gpu
POISON = 0xA5


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                                 # a copy: the shared clips are read-only


@functools.lru_cache(maxsize=None)
def clip(C):
    """(2, 37, 53, C): tail lanes, several strips, two frames (the second frame's row 0 has zeros above it, not the first frame's last row)"""
    base = gif_ref.synthetic_clip(2, 37, 53, 3)
    frames = {1: base[..., 1:2], 3: base, 4: np.concatenate([base, 255 - base[..., :1]], axis=3)}[C].copy()
    frames[0, 5, :9] = 255                                                       # bytes that wrap: 255 next to 0
    frames[0, 5, 9:18] = 0
    frames[1, 0, ::2] = 0
    frames[1, 0, 1::2] = 255
    frames.setflags(write=False)
    return frames


def every_type_wins(C):
    """(1, 8, 24, C): rows built so that each of the five filter types is the adaptive choice at least once"""
    W = 24
    rng = np.random.default_rng(40 + C)
    f = np.zeros((8, W * C), np.int64)                                           # row 0: zeros, a five-way tie: type 0
    f[1] = 7 * (np.arange(W * C) // C) + 3                                       # a ramp along the row: Sub (Paeth ties with it, Sub is lower)
    f[2] = f[1] + rng.integers(-1, 2, W * C)                                     # the row above with a little noise: Up
    for j in range(W * C):                                                       # exactly the average of left and above: Average
        f[3, j] = ((f[3, j - C] if j >= C else 0) + f[2, j]) // 2
    f[4] = 20 + np.cumsum(np.where(np.arange(W) % 2, 8, 0))[np.arange(W * C) // C]      # steps of 0 and 8 along the row ..
    f[5] = f[4] + 5                                                              # .. and of 5 down: the nearer neighbour is Paeth's
    f[6] = rng.integers(60, 200, W * C)
    f[7] = np.where((np.arange(W * C) // C) % 2 == 0, 1, 255)                    # +1, -1 behind a noisy row: None; 255 next to 1 wraps under Sub
    return (f % 256).astype(np.uint8).reshape(1, 8, W, C)


@functools.lru_cache(maxsize=None)
def filter_cases(C):
    rng = np.random.default_rng(C)
    cases = {"clip": clip(C), "pixel": rng.integers(1, 256, (1, 1, 1, C), dtype=np.uint8), "column": rng.integers(0, 256, (1, 5, 1, C), dtype=np.uint8),
             "types": every_type_wins(C)}
    return cases


@functools.lru_cache(maxsize=None)
def filtered_ref(C, name, filter):
    f = R.filter_frames(filter_cases(C)[name], filter)
    f.setflags(write=False)
    return f


# ------------------------------------------------------------------------------------------------------------------------------ filter
@pytest.mark.parametrize("filter", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_filter_equals_the_reference(C, filter):
    o = ops()
    for name, frames in filter_cases(C).items():
        want = filtered_ref(C, name, filter)
        got, adler = o.png_filter(dev(frames), filter)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape and tuple(adler.shape) == want.shape[:2] + (2,)
        assert np.array_equal(got.cpu().numpy(), want), (name, C, filter)
        assert np.array_equal(adler.cpu().numpy().astype(np.int64), R.adler_pairs(want)), (name, C, filter)
        for f in range(len(frames)):
            assert V.adler32_combine(adler[f].cpu().numpy(), want.shape[-1]) == zlib.adler32(want[f].tobytes())


@pytest.mark.parametrize("C", [1, 3, 4])
def test_adaptive_choice(C):
    want = filtered_ref(C, "types", 5)
    assert set(want[0, :, 0].tolist()) == {0, 1, 2, 3, 4} and want[0, 0, 0] == 0 and not want[0, 0].any()      # the all-zero row: a tie, type 0
    both = filtered_ref(C, "clip", 5)
    assert len(set(both[:, :, 0].reshape(-1).tolist())) >= 3
    for filter in (2, 3, 4):                                                     # row 0 of BOTH frames under Up / Average / Paeth: zeros above
        rows = filtered_ref(C, "clip", filter)
        assert np.array_equal(rows[1, 0, 1:], R.filter_row(filter, clip(C)[1, 0].reshape(-1), np.zeros(53 * C, np.uint8), C))


# ------------------------------------------------------------------------------------------------------------------------------ tokens
def colliding_triples():
    """two different byte triples with one hash slot and different first bytes"""
    seen = {}
    for v in range(1, 1 << 24):
        t = bytes([(v * 7) & 255, (v >> 8) & 255, (v >> 16) & 255])
        h = R.hash3(t, 0)
        if h in seen and seen[h][0] != t[0] and seen[h] != t:
            return seen[h], t
        seen.setdefault(h, t)
    raise AssertionError("no collision")


@functools.lru_cache(maxsize=None)
def token_cases():
    """name -> (bytes uint8 (n, H, R) standing in for filtered scanlines, channels, strip_rows)"""
    rng = np.random.default_rng(9)
    row = rng.integers(0, 256, 61, dtype=np.uint8)
    t1, t2 = colliding_triples()
    near_limit = np.tile(rng.integers(0, 256, 997, dtype=np.uint8), 61)[:60001]
    near_limit[30000:30700] = rng.integers(0, 256, 700, dtype=np.uint8)
    return {
        "random": (rng.integers(0, 256, (2, 6, 61), dtype=np.uint8), 3, 4),                       # almost all literals; a short last strip
        "flat_one_strip": (np.zeros((1, 8, 301), np.uint8), 3, 8),                                # 258-byte matches, the last capped at the strip's end
        "flat_rows": (np.full((1, 5, 31), 7, np.uint8), 1, 1),                                    # one match per strip, all at distance 1
        "repeated_rows": (np.tile(row, (1, 9, 1)), 3, 9),                                         # the row above: a distance of one row
        "repeated_rows_cut": (np.tile(row, (1, 9, 1)), 3, 1),                                     # the same bytes on both sides of every boundary
        "repeated_rows_8": (np.tile(row, (2, 19, 1)), 3, 8),                                      # strips of 8, 8 and 3 rows
        "two_bytes": (np.array([[[0, 200]]], np.uint8), 1, 8),                                    # nothing to hash
        "shared_slot": (np.frombuffer(t1 + t2 + t1, np.uint8).reshape(1, 1, 9).copy(), 1, 1),     # the probe must compare the bytes
        "near_limit": (near_limit.reshape(1, 1, 60001), 1, 1),                                    # 60001 bytes in one strip: more than 64 KiB of LDS
    }


@functools.lru_cache(maxsize=None)
def token_ref(name):
    data, C, rows = token_cases()[name]
    return [R.tokenize_frame(f, rows) for f in data]


@pytest.mark.parametrize("name", sorted(token_cases()))
def test_tokens_equal_the_reference(name):
    data, C, rows = token_cases()[name]
    o = ops()
    tokens, n_tokens, hist = o.png_lz_count(dev(data), C, rows)
    n, H, Rb = data.shape
    strips = -(-H // min(rows, H))
    assert tuple(tokens.shape) == (n, strips, min(rows, H) * Rb) and tuple(n_tokens.shape) == (n, strips) and tuple(hist.shape) == (n, 320)
    tok, cnt, hst = tokens.cpu().numpy().view(np.uint32), n_tokens.cpu().numpy(), hist.cpu().numpy()
    for f, (want, want_hist) in enumerate(token_ref(name)):
        assert len(want) == strips
        for s, w in enumerate(want):
            assert cnt[f, s] == len(w) and np.array_equal(tok[f, s, :len(w)], R.packed(w)), (name, f, s)
        assert np.array_equal(hst[f], want_hist) and hst[f, 256] == 1, (name, f)
    want, want_hist = token_ref(name)[0]
    matches = [t for w in want for t in w if isinstance(t, tuple)]
    if name == "random":
        assert len(matches) <= 2
    elif name == "flat_one_strip":      # literal, 258 at distance 1, then the slot holds offset 1: 258 at distance 258, and what is left
        assert want[0][:3] == [0, (258, 1), (258, 258)] and want[0][-1][0] == (8 * 301 - 1) % 258 and sum(t[0] for t in matches) == 8 * 301 - 1
    elif name == "flat_rows":
        assert all(w == [7, (30, 1)] for w in want) and np.flatnonzero(want_hist[288:]).tolist() == [0]      # exactly one distance symbol
    elif name == "repeated_rows":
        assert matches[0] == (258, 61) and all(t[1] % 61 == 0 for t in matches) and sum(t[0] for t in matches) == 8 * 61
    elif name == "repeated_rows_cut":
        assert len(matches) <= 1 and [len(w) for w in want].count(61) >= 8       # no match crosses into the strip above
    elif name == "repeated_rows_8":
        assert [sum(t[0] if isinstance(t, tuple) else 1 for t in w) for w in want] == [8 * 61, 8 * 61, 3 * 61]
    elif name == "two_bytes":
        assert want == [[0, 200]]
    elif name == "shared_slot":
        assert want == [list(data.reshape(-1))]                                  # nine literals
    elif name == "near_limit":
        assert matches[0] == (258, 997) and all(t[1] % 997 == 0 for t in matches[:30]) and sum(t[0] if isinstance(t, tuple) else 1 for t in want[0]) == 60001


# ------------------------------------------------------------------------------------------------------------------------------ stream
def stream_cases():
    rng = np.random.default_rng(12)
    phases = rng.integers(0, 4, (3, 5, 7, 3), dtype=np.uint8)
    phases[1, 2:] = 1
    phases[2] = 3
    return {"clip1": (clip(1), 8), "clip3": (clip(3), 8), "clip4": (clip(4), 5), "clip3_rows": (clip(3), 1), "clip3_whole": (clip(3), None),
            "types3": (every_type_wins(3), 3), "pixel": (np.array([[[[9]]]], np.uint8), 8), "column": (filter_cases(4)["column"], 2),
            "flat": (np.full((1, 40, 40, 3), 201, np.uint8), 8), "flat_rows": (np.full((1, 3, 20, 1), 7, np.uint8), 1),
            "random": (rng.integers(0, 256, (2, 9, 11, 3), dtype=np.uint8), 4), "phases": (phases, 2)}


def device_streams(frames, filter, strip_rows, poison=False):
    """png_zlib_streams step by step, with the scratch tokens behind n_tokens and the bytes around the stream buffer poisoned"""
    o = ops()
    n, H, W, C = frames.shape
    rows = V.png_strip_rows(strip_rows, H, W, C)
    filtered, adler = o.png_filter(dev(frames), filter)
    tokens, n_tokens, hist = o.png_lz_count(filtered, C, rows)
    if poison:
        cap = tokens.shape[2]
        behind = torch.arange(cap, device=DEV)[None, None, :] >= n_tokens[:, :, None]
        tokens = torch.where(behind, torch.full_like(tokens, -0x5A5A5A5B), tokens).contiguous()      # 0xA5A5A5A5
    hist_host = hist.cpu().numpy()
    tables = [V.deflate_tables(h) for h in hist_host]
    codes = torch.from_numpy(np.stack([t.codes for t in tables]).view(np.int32)).to(DEV)
    bits = o.png_deflate_bits(tokens, n_tokens, codes, H, W, C, rows)
    token_bits = np.array([t.token_bits(h) for t, h in zip(tables, hist_host)], np.int64)
    assert np.array_equal(bits.cpu().numpy().astype(np.int64).sum(axis=1), token_bits)      # the sizes the host derives from the histogram
    head = np.array([16 + t.header_bits for t in tables], np.int64)
    ends_bits = head + token_bits + np.array([t.end_of_block[1] for t in tables], np.int64)
    nbytes = (ends_bits + 7) // 8 + 4
    starts = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    ends = torch.cumsum(bits, dim=1, dtype=torch.int64)
    offsets = (ends - bits + torch.from_numpy(starts * 8 + head).to(DEV)[:, None]).contiguous()
    total = int(nbytes.sum())
    words = (total + 3) // 4 * 4
    buf = torch.full((64 + words + 64,), POISON, device=DEV, dtype=torch.uint8)
    buf[64:64 + total] = 0
    o.png_deflate_emit(tokens, n_tokens, codes, offsets, buf[64:64 + words], H, W, C, rows)
    host = buf.cpu().numpy()
    assert bool((host[:64] == POISON).all()) and bool((host[64 + total:] == POISON).all())
    body = host[64:64 + total]
    streams = [V.zlib_stream(body[s:s + b], t, tb, V.adler32_combine(a, 1 + W * C))
               for s, b, t, tb, a in zip(starts, nbytes, tables, token_bits, adler.cpu().numpy())]
    return streams, ends_bits, (tokens, n_tokens, codes, offsets, rows)


@pytest.mark.parametrize("name", sorted(stream_cases()))
def test_streams_and_files_equal_the_reference(name):
    frames, strip_rows = stream_cases()[name]
    n, H, W, C = frames.shape
    filtered, files = R.reference_files(frames, 5, strip_rows, V.deflate_tables)
    streams, ends_bits, _ = device_streams(frames, 5, strip_rows, poison=True)
    got = V.encode_png(dev(frames), strip_rows=strip_rows)
    assert got == V.encode_png(dev(frames), strip_rows=strip_rows)               # integer atomics: the same bytes every run
    for f in range(n):
        assert R.first_block_type(streams[f]) == (1, 2)
        assert zlib.decompress(streams[f]) == filtered[f].tobytes(), (name, f)
        assert R.parse_chunks(got[f])[1] == (b"IDAT", streams[f]) and got[f] == files[f], (name, f)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(got[f]))).reshape(H, W, C), frames[f]), (name, f)
    if name == "phases":
        assert len({int(e) % 8 for e in ends_bits}) == 3                         # frames start on bytes, their blocks end inside one
    if name == "flat_rows":
        assert V.deflate_tables(R.tokenize_frame(filtered[0], 1)[1]).lengths[288:].tolist() == [1] + [0] * 31      # one distance code: one bit


@pytest.mark.parametrize("filter", ["none", "sub", "up", "average", "paeth"])
def test_forced_filters_make_files(filter):
    frames = clip(3)
    code = ops().PNG_FILTERS[filter]
    filtered, files = R.reference_files(frames, code, V.PNG_STRIP_ROWS, V.deflate_tables)
    assert (filtered[:, :, 0] == code).all()
    assert V.encode_png(dev(frames), filter=filter) == files


def test_emit_touches_nothing_outside_its_streams():
    o = ops()
    frames = stream_cases()["random"][0]
    n, H, W, C = frames.shape
    _, _, (tokens, n_tokens, codes, offsets, rows) = device_streams(frames, 5, 4)
    fresh = torch.full((64,), POISON, device=DEV, dtype=torch.uint8)             # offsets that point outside the buffer write nothing at all
    o.png_deflate_emit(tokens, n_tokens, codes, offsets + 8 * 64, fresh, H, W, C, rows)
    o.png_deflate_emit(tokens, n_tokens, codes, offsets - 8 * 65536, fresh, H, W, C, rows)
    o.png_deflate_emit(tokens, torch.full_like(n_tokens, -1), codes, offsets * 0, fresh, H, W, C, rows)      # counts the first pass cannot leave
    o.png_deflate_emit(tokens, torch.full_like(n_tokens, 1 << 20), codes, offsets * 0, fresh, H, W, C, rows)
    assert bool((fresh == POISON).all())
    with pytest.raises(EmoHipError, match="multiple of 4"):
        o.png_deflate_emit(tokens, n_tokens, codes, offsets, torch.zeros(30, device=DEV, dtype=torch.uint8), H, W, C, rows)
    with pytest.raises(EmoHipError):
        V.encode_png(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))                 # host frames: no CPU path


def test_shape_refusals():
    """the entries check their shapes before anything is launched"""
    lib = _lib.load()
    o = ops()
    buf = dev(np.zeros(64, np.uint8))
    p, none = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(0)
    for n, H, W, C, match in ((1, 4, 4, 2, "C=2"), (1, 0, 4, 3, "at least 1"), (1, 4, 0, 3, "at least 1"), (0, 4, 4, 3, "at least 1"),
                              (1, 1, 2 ** 31 - 1, 1, "31 bits"), (1, 2 ** 20, 2 ** 11, 1, "31 bits"), (1, 2, 2 ** 29, 4, "31 bits")):
        with pytest.raises(EmoHipError, match=match):
            _lib.check(lib.emo_png_filter(p, p, p, n, H, W, C, 5, none), "emo_png_filter")
        with pytest.raises(EmoHipError, match=match):
            _lib.check(lib.emo_png_lz_count(p, p, p, p, n, H, W, C, 1, none), "emo_png_lz_count")
    with pytest.raises(EmoHipError, match="filter=6"):
        _lib.check(lib.emo_png_filter(p, p, p, 1, 4, 4, 3, 6, none), "emo_png_filter")
    for entry, args in (("emo_png_lz_count", (p, p, p, p)), ("emo_png_deflate_bits", (p, p, p, p))):
        with pytest.raises(EmoHipError, match="65535 bytes per strip"):
            _lib.check(getattr(lib, entry)(*args, 1, 64, 341, 3, 64, none), entry)      # 64 rows of 1024 bytes: 65536
        with pytest.raises(EmoHipError, match="strip_rows=0"):
            _lib.check(getattr(lib, entry)(*args, 1, 64, 341, 3, 0, none), entry)
    with pytest.raises(EmoHipError, match="65535 bytes per strip"):
        _lib.check(lib.emo_png_deflate_emit(p, p, p, p, p, 64, 1, 64, 341, 3, 64, none), "emo_png_deflate_emit")
    with pytest.raises(EmoHipError, match="65535 bytes per strip"):
        o.png_lz_count(dev(np.zeros((1, 64, 1024), np.uint8)), 3, 64)
    assert lib.emo_png_tokens_per_strip(64, 341, 3, 63) == 63 * 1024 and lib.emo_png_tokens_per_strip(5, 4, 4, 8) == 5 * 17
    assert lib.emo_png_tokens_per_strip(5, 4, 2, 8) == 0
    # the wrapper lowers strip_rows instead: the same frame goes through in strips of 63 rows
    frames = np.random.default_rng(2).integers(0, 4, (1, 64, 341, 3), dtype=np.uint8)
    assert V.png_strip_rows(64, 64, 341, 3) == 63
    data = V.encode_png(dev(frames), strip_rows=None)[0]
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), frames[0])


# ------------------------------------------------------------------------------------------------------------------------------ surface
def decoded_apng(data):
    im = Image.open(io.BytesIO(data))
    frames, durations = [], []
    for i in range(getattr(im, "n_frames", 1)):
        im.seek(i)
        frames.append(np.asarray(im.convert("RGB" if im.mode not in ("L", "RGBA") else im.mode)))
        durations.append(im.info.get("duration"))
    return np.stack(frames), durations, im.info.get("loop")


def test_encode_apng():
    frames = stream_cases()["phases"][0]
    data = V.encode_apng(dev(frames), Fraction(30000, 1001), loop=2, strip_rows=2)
    got, durations, loop = decoded_apng(data)
    assert got.shape == frames.shape and np.array_equal(got, frames) and loop == 2
    assert durations == [pytest.approx(1001000 / 30000)] * 3
    stills = V.encode_png(dev(frames), strip_rows=2)
    chunks = R.parse_chunks(data)
    assert [k for k, _ in chunks] == [b"IHDR", b"acTL", b"fcTL", b"IDAT", b"fcTL", b"fdAT", b"fcTL", b"fdAT", b"IEND"]
    assert chunks[3][1] == R.parse_chunks(stills[0])[1][1] and chunks[7][1][4:] == R.parse_chunks(stills[2])[1][1]
    assert V.encode_apng(dev(frames)[None], Fraction(30000, 1001), loop=2, strip_rows=2) == data      # the (1, n, H, W, 3) of output_type="uint8"
    grey = clip(1)
    got, durations, loop = decoded_apng(V.encode_apng(dev(grey), 25))
    assert np.array_equal(got, grey[..., 0]) and durations == [40.0, 40.0] and loop == 0


def test_write_png_and_the_reference_surface(tmp_path):
    frames = clip(3)
    paths = V.write_png(dev(frames), tmp_path / "sub" / "frame_%04d.png", filter="paeth")      # the directory is made
    assert [p.rsplit("/", 1)[1] for p in paths] == ["frame_0000.png", "frame_0001.png"]
    for p, want in zip(paths, frames):
        assert np.array_equal(np.asarray(Image.open(p)), want)
    one = tmp_path / "one.png"
    assert V.write_png(dev(frames[1]), one) == [str(one)]                        # (H, W, C): one frame
    assert one.read_bytes() == V.encode_png(dev(frames[1:]))[0] and np.array_equal(np.asarray(Image.open(one)), frames[1])
    with pytest.raises(ValueError, match=r"%04d.*\.apng"):
        V.write_png(dev(frames), tmp_path / "two.png")
    # save_images_grid: the grid of make_grid_u8 at torchvision's defaults, lossless or as one JPEG frame
    images = torch.rand(10, 3, 1, 9, 6, generator=torch.Generator().manual_seed(3))
    grid = V.make_grid_u8(images.to(DEV), n_rows=8)
    assert tuple(grid.shape) == (1, 2 * 11 + 2, 8 * 8 + 2, 3)
    V.save_images_grid(images, str(tmp_path / "grids" / "grid.png"))
    assert np.array_equal(np.asarray(Image.open(tmp_path / "grids" / "grid.png")), grid[0].cpu().numpy())
    V.save_images_grid(images, str(tmp_path / "grid.jpg"))
    assert (tmp_path / "grid.jpg").read_bytes() == V.encode_mjpeg(grid)[0]
    assert np.array_equal(np.asarray(Image.open(tmp_path / "grid.jpg").convert("RGB")), V.decode_jpeg(V.encode_mjpeg(grid)[0]))
    single = torch.rand(1, 1, 1, 5, 4, generator=torch.Generator().manual_seed(4))      # b == 1: the image itself; one channel is repeated
    V.save_images_grid(single, str(tmp_path / "single.png"))
    want = (single[0, 0, 0] * 255).to(torch.uint8).numpy()
    assert np.array_equal(np.asarray(Image.open(tmp_path / "single.png")), np.repeat(want[..., None], 3, axis=2))
    # write_video / save_videos_grid / images2video with format="apng"
    videos = torch.rand(3, 3, 4, 10, 6, generator=torch.Generator().manual_seed(5))
    path = tmp_path / "v" / "grid.apng"
    V.save_videos_grid(videos, str(path), n_rows=2, fps=8, format="apng", loop=1)
    vgrid = V.make_grid_u8(videos.to(DEV), n_rows=2)
    got, durations, loop = decoded_apng(path.read_bytes())
    assert np.array_equal(got, vgrid.cpu().numpy()) and durations == [125.0] * 4 and loop == 1
    direct = tmp_path / "direct.apng"
    V.write_video(vgrid, direct, 8, format="apng", loop=1)
    assert direct.read_bytes() == path.read_bytes()
    V.images2video([f for f in vgrid.cpu().numpy()], str(tmp_path / "frames.apng"), format="apng", filter="up", strip_rows=3)
    got, durations, loop = decoded_apng((tmp_path / "frames.apng").read_bytes())
    assert np.array_equal(got, vgrid.cpu().numpy()) and durations == [125.0] * 4 and loop == 0      # images2video's default rate


def test_call_save_path_writes_png_files(tmp_path, monkeypatch):
    from tests.test_gpu_gif import F_TOT, LOOP_KW                                # the tiny pipeline of the GIF test
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    from emote_hack_amd.synth import seeded_randn
    from tests import cases
    from tests.test_gpu_unet import build
    from tests.test_gpu_vae import SMALL, build as build_vae
    ref = build(cases.TINY, torch.float32, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    pipe = EMOAnimationPipeline(vae=build_vae(SMALL, torch.float32)[0], unet=build(cases.TINY_MOTION, torch.float32), scheduler=DDIMScheduler())
    kw = dict(video_length=F_TOT, height=128, width=128, latents=seeded_randn((1, 4, F_TOT, 16, 16), 5).to(DEV),
              text_embeddings=seeded_randn((2, 5, 32), 2), ref_image_latents=seeded_randn((1, 4, 16, 16), 3), appearance_encoder=ref,
              audio_features=seeded_randn((F_TOT, 5, 32), 7), **LOOP_KW)
    plain = pipe("", output_type="uint8", **kw).videos
    want = plain[0].cpu().numpy()
    path = tmp_path / "clip.apng"
    got = pipe("", output_type="uint8", fps=8, save_path=str(path), save_loop=3, save_png_filter="paeth", **kw).videos
    assert torch.equal(got, plain) and tuple(got.shape) == (1, F_TOT, 128, 128, 3)      # the return value is what it is without save_path
    frames, durations, loop = decoded_apng(path.read_bytes())
    assert np.array_equal(frames, want) and durations == [125.0] * F_TOT and loop == 3
    assert path.read_bytes() == V.encode_apng(plain, 8, loop=3, filter="paeth")
    stills = tmp_path / "frames" / "f_%04d.png"
    again = pipe("", output_type="uint8", save_path=str(stills), **kw).videos      # numbered stills: no fps=
    assert torch.equal(again, plain)
    assert sorted(p.name for p in (tmp_path / "frames").iterdir()) == [f"f_{i:04d}.png" for i in range(F_TOT)]
    for i in range(F_TOT):
        assert np.array_equal(np.asarray(Image.open(str(stills) % i)), want[i]), i
    twice = pipe("", output_type="uint8", interpolation_factor=2, fps=8, save_path=tmp_path / "twice.apng", **kw).videos
    frames, durations, loop = decoded_apng((tmp_path / "twice.apng").read_bytes())
    assert np.array_equal(frames, twice[0].cpu().numpy()) and durations == [62.5] * ((F_TOT - 1) * 2 + 1) and loop == 0
    # an `.avi` path still goes the way it went: the same bytes, and none of the PNG kernels
    o = ops()

    def never(*a, **k):
        raise AssertionError("a PNG kernel on the way to an `.avi` file")
    for name in ("png_filter", "png_lz_count", "png_deflate_bits", "png_deflate_emit"):
        monkeypatch.setattr(o, name, never)
    avi = tmp_path / "clip.avi"
    third = pipe("", output_type="uint8", fps=8, save_path=str(avi), **kw).videos
    jpegs, fps, audio = V.read_avi(avi)
    assert torch.equal(third, plain) and fps == 8 and audio is None and jpegs == V.encode_mjpeg(plain, 90)
