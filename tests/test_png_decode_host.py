"""Host tests of the PNG reader: the serial reference of tests/png_decode_ref.py against zlib on every stream the GPU tests run, the
claims those tests make about their inputs (asserted from the reference's record, so no test claims a case its input does not hold),
and parse_png on files of Pillow and of this project's own container functions, every refusal by name."""
import io
import struct
import zlib
from fractions import Fraction

import numpy as np
import pytest
from PIL import Image

from emote_hack_amd import video_io as V
from tests import png_decode_cases as K
from tests import png_decode_ref as D
from tests import png_ref


# ------------------------------------------------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize("name", sorted(K.all_streams()))
def test_reference_equals_zlib(name):
    stream, data = K.all_streams()[name]
    assert K.raw_inflate(stream) == data
    out, status, _ = D.inflate(stream, len(data))
    assert status == D.OK and out == data
    assert D.inflate(stream)[:2] == (data, D.OK)


@pytest.mark.parametrize("name", sorted(K.damaged_streams()))
def test_reference_reports_what_zlib_refuses(name):
    stream, status = K.damaged_streams()[name]
    out, got, _ = D.inflate(stream, K.SMALL)
    assert got == status and got != D.OK
    if status in (D.OVERFLOW, D.SHORT):                                          # a sound stream for a frame of another size
        assert len(K.raw_inflate(stream)) != K.SMALL
    else:
        with pytest.raises(zlib.error):
            K.raw_inflate(stream)


def test_every_status_has_a_damaged_stream():
    assert {s for _, s in K.damaged_streams().values()} == set(range(1, 9))


def test_the_streams_hold_what_the_gpu_tests_claim():
    rec = {k: D.inflate(s)[2] for k, (s, _) in K.all_streams().items()}
    assert rec["pillow_noise64"]["blocks"] == [0]                                 # one stored block
    assert rec["pillow_noise160"]["blocks"].count(0) >= 2 and K.pillow_files()["noise160"].count(b"IDAT") == 2
    assert rec["pillow_tiny"]["blocks"] == [1]
    for k in ("pillow_flat", "pillow_gradient"):
        assert rec[k]["blocks"] == [2] and rec[k]["distances"]
    assert 1 in rec["pillow_flat"]["distances"]                                   # a run: the match overlaps itself
    for k in ("flushes6", "flushes1"):
        assert rec[k]["empty_stored"] >= 3
    # stored blocks whose header ends on bit 2, 3, 5, 6 of a byte: the skip to the next byte is 6, 5, 3, 2 bits
    assert {2, 3, 5, 6} <= rec["flushes6"]["stored_bit_positions"] | rec["flushes1"]["stored_bit_positions"]
    assert 1 in rec["flushes1"]["blocks"] and 2 in rec["flushes1"]["blocks"]
    assert rec["level1"]["blocks"] and rec["level9"]["blocks"]
    assert {3, 64, 65, 128, 129, 258} <= rec["lengths"]["lengths"] and {1, 2, 3, 63, 64, 65} <= rec["lengths"]["distances"]
    assert rec["whole_history"]["whole_history"] and rec["far_dest"]["whole_history"]
    assert rec["far_dest"]["dest_crosses"] and 7 in rec["far_dest"]["stored_bit_positions"]
    assert rec["far_source"]["stored_crosses"] and rec["far_source"]["source_crosses"] and 32768 in rec["far_source"]["distances"]
    assert rec["code15"]["longest_code"] == 15 and rec["code15"]["no_distance_codes"]
    assert rec["one_distance"]["one_code_distance_set"] and rec["one_distance"]["distances"] == {1}
    assert rec["repeat_crosses"]["repeat_crosses"]
    assert max(max(r["distances"], default=0) for k, r in rec.items() if not k.startswith(("far", "lengths"))) <= 32506
    for k in ("far_dest", "far_source"):
        assert len(K.all_streams()[k][1]) == K.FAR == 130 * (1 + 257)


def test_unfilter_reference_undoes_the_filter_reference():
    rng = np.random.default_rng(3)
    for C in (1, 2, 3, 4):
        frames = rng.integers(0, 256, (2, 5, 7, C), dtype=np.uint8)
        for t in range(6):
            filtered = png_ref.filter_frames(frames, t)
            assert np.array_equal(D.unfilter(filtered, C), frames)
    with pytest.raises(ValueError):
        D.unfilter(np.full((1, 1, 3), 5, np.uint8), 1)


# ------------------------------------------------------------------------------------------------------------------------------ parse_png
def _pillow(array, **options):
    return K.pillow_file(array, **options)


@pytest.mark.parametrize("mode,C", [("L", 1), ("LA", 2), ("RGB", 3), ("RGBA", 4)])
def test_parse_png_reads_pillow_files(mode, C):
    a = K.noise((9, 13, C), C) if C > 1 else K.noise((9, 13), C)
    f = _pillow(a)
    p = V.parse_png(f)
    assert (p.height, p.width, p.channels, p.animated, len(p.frames)) == (9, 13, C, False, 1)
    filtered = np.frombuffer(K.raw_inflate(p.still), np.uint8).reshape(1, 9, 1 + 13 * C)
    assert zlib.adler32(filtered.tobytes()) == p.still_adler
    assert np.array_equal(D.unfilter(filtered, C)[0].reshape(a.shape), np.asarray(Image.open(io.BytesIO(f))))


def test_parse_png_skips_ancillary_chunks_and_trns_as_pillow_does():
    from PIL import PngImagePlugin
    info = PngImagePlugin.PngInfo()
    info.add_text("comment", "x" * 50)
    grey, rgb = K.noise((4, 5), 1), K.noise((4, 5, 3), 2)
    for a, trns in ((grey, 7), (rgb, (1, 2, 3))):
        f = _pillow(a, pnginfo=info, transparency=trns, dpi=(72, 72))
        assert b"tRNS" in f and b"tEXt" in f and b"pHYs" in f
        p = V.parse_png(f)
        im = Image.open(io.BytesIO(f))
        assert np.array_equal(np.asarray(im), a)                                 # Pillow leaves the samples of a tRNS file as they are ..
        assert np.array_equal(np.asarray(im.convert("RGB")), a if a.ndim == 3 else np.repeat(a[..., None], 3, 2))     # .. in RGB too
        filtered = np.frombuffer(K.raw_inflate(p.still), np.uint8).reshape(1, 4, -1)
        assert np.array_equal(D.unfilter(filtered, p.channels)[0].reshape(a.shape), a)


def _own_streams(frames):
    return [zlib.compress(png_ref.filter_frames(f[None], 5).tobytes(), 6) for f in frames]


def test_parse_png_reads_this_projects_containers():
    frames = K.noise((3, 6, 7, 3), 4)
    streams = _own_streams(frames)
    p = V.parse_png(V.png_container(7, 6, 3, streams[0]))
    assert (p.height, p.width, p.channels, p.animated, p.delays, p.loop) == (6, 7, 3, False, (), 0)
    assert p.still == streams[0][2:-4] and p.still_adler == struct.unpack(">I", streams[0][-4:])[0]
    p = V.parse_png(V.apng_container(7, 6, 3, streams, Fraction(30000, 1001), loop=2))
    assert p.animated and p.still_in_animation and p.loop == 2 and p.delays == (Fraction(1001, 30000),) * 3
    assert [s for s, _ in p.frames] == [s[2:-4] for s in streams] and p.frames[0] == (p.still, p.still_adler)


def _chunks(kinds_bodies):
    return V.PNG_SIGNATURE + b"".join(V.png_chunk(k, b) for k, b in kinds_bodies)


def _ihdr(W=7, H=6, depth=8, colour=2, lace=0):
    return struct.pack(">IIBBBBB", W, H, depth, colour, 0, 0, lace)


def _fctl(seq, W=7, H=6, x=0, y=0, num=1, den=25, dispose=0, blend=0):
    return struct.pack(">IIIIIHHBB", seq, W, H, x, y, num, den, dispose, blend)


def test_parse_png_default_image_outside_the_animation_and_split_data():
    s = _own_streams(K.noise((3, 6, 7, 3), 5))
    f = _chunks([(b"IHDR", _ihdr()), (b"acTL", struct.pack(">II", 2, 0)), (b"IDAT", s[0][:10]), (b"IDAT", s[0][10:]), (b"fcTL", _fctl(0, den=0)),
                 (b"fdAT", struct.pack(">I", 1) + s[1][:5]), (b"fdAT", struct.pack(">I", 2) + s[1][5:]), (b"fcTL", _fctl(3, num=3, den=50)),
                 (b"fdAT", struct.pack(">I", 4) + s[2]), (b"IEND", b"")])
    p = V.parse_png(f)
    assert p.animated and not p.still_in_animation and p.still == s[0][2:-4]
    assert [x for x, _ in p.frames] == [s[1][2:-4], s[2][2:-4]] and p.delays == (Fraction(1, 100), Fraction(3, 50))


def _refused(file, *words):
    with pytest.raises(ValueError) as e:
        V.parse_png(file)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_parse_png_refusals_by_name():
    s = _own_streams(K.noise((2, 6, 7, 3), 6))
    good = V.png_container(7, 6, 3, s[0])
    V.parse_png(good)
    _refused(b"JFIF" + good, "signature")
    _refused(_pillow(K.noise((4, 4), 1).astype(np.uint16) * 257), "bit depth 16")
    palette = io.BytesIO()
    Image.fromarray(K.noise((4, 4, 3), 2)).convert("P").save(palette, "PNG")
    _refused(palette.getvalue(), "palette")
    _refused(_pillow(K.noise((4, 4), 3) > 127), "bit depth 1")
    _refused(_chunks([(b"IHDR", _ihdr(lace=1)), (b"IDAT", s[0]), (b"IEND", b"")]), "interlaced", "Adam7")
    apng = lambda **k: _chunks([(b"IHDR", _ihdr()), (b"acTL", struct.pack(">II", 2, 0)), (b"fcTL", _fctl(0)), (b"IDAT", s[0]),
                                (b"fcTL", _fctl(1, **k)), (b"fdAT", struct.pack(">I", 2) + s[1]), (b"IEND", b"")])
    V.parse_png(apng())
    _refused(apng(W=3, H=2, x=1, y=1), "partial frame")
    _refused(apng(blend=1), "blend_op 1")
    flipped = bytearray(good)
    flipped[45] ^= 1
    _refused(bytes(flipped), "CRC mismatch", "IDAT")
    _refused(good[:-12], "IEND")
    _refused(good[:-5], "IEND")
    _refused(_chunks([(b"IHDR", _ihdr()), (b"ABCD", b"xy"), (b"IDAT", s[0]), (b"IEND", b"")]), "unknown critical chunk", "ABCD")
    V.parse_png(_chunks([(b"IHDR", _ihdr()), (b"abCD", b"xy"), (b"IDAT", s[0]), (b"IEND", b"")]))
    _refused(_chunks([(b"IHDR", _ihdr()), (b"acTL", struct.pack(">II", 2, 0)), (b"fcTL", _fctl(0)), (b"IDAT", s[0]), (b"fcTL", _fctl(1)),
                      (b"fdAT", struct.pack(">I", 3) + s[1]), (b"IEND", b"")]), "sequence number 3")
    _refused(_chunks([(b"IHDR", _ihdr()), (b"acTL", struct.pack(">II", 3, 0)), (b"fcTL", _fctl(0)), (b"IDAT", s[0]), (b"IEND", b"")]), "acTL counts 3")
    _refused(_chunks([(b"IHDR", _ihdr()), (b"IDAT", s[0][:9]), (b"tEXt", b"a\0b"), (b"IDAT", s[0][9:]), (b"IEND", b"")]), "not consecutive")
    _refused(_chunks([(b"IHDR", _ihdr()), (b"IEND", b"")]), "no IDAT")


@pytest.mark.parametrize("cmf,flg,word", [(0x79, 0, "compression method 9"), (0x88, 0, "window"), (0x78, None, "FCHECK"),
                                          (0x78, 0x20, "preset dictionary")])
def test_parse_png_checks_the_zlib_header(cmf, flg, word):
    s = _own_streams(K.noise((1, 6, 7, 3), 7))[0]
    if flg is None:
        header = bytes([cmf, 0x02])                                              # 0x7802 is no multiple of 31
    else:
        header = bytes([cmf, flg + (31 - (cmf << 8 | flg) % 31) % 31])         # the check bits made right: only the named field is wrong
        assert (header[0] << 8 | header[1]) % 31 == 0
    _refused(V.png_container(7, 6, 3, header + s[2:]), word)
