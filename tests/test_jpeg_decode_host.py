"""CPU tests of the Motion-JPEG reader's host half and of the restatement the GPU tests lean on.

tests/jpeg_decode_ref.py restates emo_jpeg_decode_bits / emo_jpeg_idct / emo_jpeg_rgb in numpy (the standard's serial Huffman
decoder, libjpeg's integer IDCT, its triangle chroma filter and fixed-point colour transform).  Every step is integer arithmetic, so it is
held to Pillow's decoder (libjpeg-turbo, default settings) by EQUALITY: on files framed from known coefficients and on Pillow's own files,
with the standard Huffman tables and with optimised ones.  emote_hack_amd.video_io.parse_jpeg is then checked against jpeg_header /
finish_scan, the restatement's own marker walk, and every kind of file it must refuse, each written that way by Pillow."""
import io
import struct

import numpy as np
import pytest

from emote_hack_amd import video_io as V
from tests import jpeg_decode_ref as D
from tests import mjpeg_ref as R


def framed_files(content, n, H, W, quality):
    """the n files framed from the restated encoder's coefficients of R.make_frames(content, n, H, W) -> (files, coefficients)"""
    t = V.jpeg_tables(quality)
    coefs, _ = R.blocks(R.make_frames(content, n, H, W), t.quant)
    _, streams, _ = R.entropy(coefs, t.huff)
    return [V.jpeg_header(H, W, quality) + V.finish_scan(s, b) for s, b in streams], coefs


# ------------------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("n,H,W", R.SHAPES)
def test_restatement_equals_pillow_on_files_with_known_coefficients(n, H, W, content):
    for quality in R.QUALITIES:
        files, coefs = framed_files(content, n, H, W, quality)
        for i, data in enumerate(files):
            got, want = D.decode(data), R.decode(data)
            assert got.shape == want.shape == (H, W, 3)
            assert np.array_equal(got, want), (content, n, H, W, quality, i, int(np.abs(got.astype(int) - want).max()))
            # and the entropy decoder gives back the very coefficients that were coded
            _, _, _, specs, scan = D.split_file(data)
            assert np.array_equal(D.huffman_decode(scan, specs, coefs.shape[1]), coefs[i]), (content, n, H, W, quality, i)


@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("H,W", D.PILLOW_SIZES)
def test_restatement_equals_pillow_on_pillows_own_files(H, W, optimize):
    for quality in D.PILLOW_QUALITIES:
        data = D.pillow_file(D.picture(H, W, H * W + quality), quality, optimize)
        got, want = D.decode(data), R.decode(data)
        assert np.array_equal(got, want), (H, W, quality, optimize, int(np.abs(got.astype(int) - want).max()))
    if optimize:                                               # the file carries tables of its own
        assert D.split_file(data)[3] != list(V.HUFFMAN_SPECS)


def test_restatement_reports_what_the_kernel_reports():
    files, coefs = framed_files("ramp", 1, 24, 40, 90)
    _, _, _, specs, scan = D.split_file(files[0])
    for damaged, status in ((scan[:len(scan) // 2], D.PAST_END), (np.zeros(0, np.uint8), D.PAST_END),
                            (np.concatenate([np.array([0xFF, 0xFF], np.uint8), scan]), D.BAD_CODE)):
        with pytest.raises(D.DecodeError) as e:
            D.huffman_decode(damaged, specs, coefs.shape[1])
        assert e.value.status == status
    # ZRL, ZRL, ZRL, ZRL and a coefficient: 64 zeros and one more leave the block
    code, length = V.huffman_codes(*V.HUFFMAN_SPECS[1])
    bits = "00" + 4 * format(int(code[0xF0]), f"0{int(length[0xF0])}b") + format(int(code[0x01]), f"0{int(length[0x01])}b") + "1"
    stream = np.packbits(np.array([int(b) for b in bits + "1" * (-len(bits) % 8)], np.uint8))
    with pytest.raises(D.DecodeError) as e:
        D.huffman_decode(stream, V.HUFFMAN_SPECS, 1)
    assert e.value.status == D.BAD_RUN


# ------------------------------------------------------------------------------------------------------------------------ parse_jpeg
def test_decode_tables_follow_annex_c():
    for spec in V.HUFFMAN_SPECS:
        t = V.huffman_decode_table(*spec)
        mincode, maxcode, valptr, huffval = D.code_tables(*spec)
        assert t.dtype == np.int32 and t.shape == (V.ops.JPEG_DECODE_TABLE_INTS,)
        for size in range(1, 17):
            assert t[16 + size - 1] == maxcode[size]
            if maxcode[size] >= 0:
                assert t[size - 1] == mincode[size] and t[32 + size - 1] == valptr[size]
        assert bytes(t[64:64 + len(huffval)].astype(np.uint8)) == huffval and not t[64 + len(huffval):].any()
        # every symbol's code, looked up the decoder's way, gives the symbol back
        code, length = V.huffman_codes(*spec)
        for sym in spec[1]:
            size = int(length[sym])
            assert t[size - 1] <= code[sym] <= t[16 + size - 1] and t[64 + t[32 + size - 1] + int(code[sym]) - t[size - 1]] == sym
    with pytest.raises(ValueError, match="over-subscribed"):
        V.huffman_decode_table((3,) + (0,) * 15, bytes(3))
    with pytest.raises(ValueError):
        V.huffman_decode_table((1,) + (0,) * 15, bytes(2))


@pytest.mark.parametrize("quality", R.QUALITIES)
def test_parse_jpeg_reverses_header_and_finish_scan(quality):
    n, H, W = 3, 70, 38
    t = V.jpeg_tables(quality)
    coefs, _ = R.blocks(R.make_frames("noise", n, H, W), t.quant)
    _, streams, _ = R.entropy(coefs, t.huff)
    stuffed = 0
    for stream, bits in streams:
        data = V.jpeg_header(H, W, quality) + V.finish_scan(stream, bits)
        p = V.parse_jpeg(data)
        assert (p.height, p.width) == (H, W) and p.quant.dtype == np.uint16 and np.array_equal(p.quant, t.quant) and p.specs == tuple(t.specs)
        want = np.array(stream[:(bits + 7) // 8], np.uint8)
        if bits & 7:
            want[-1] |= (1 << (8 - (bits & 7))) - 1                              # the 1-bits that fill the last byte stay in the scan
        assert p.scan.dtype == np.uint8 and np.array_equal(p.scan, want)
        stuffed += int((want == 0xFF).sum())
        assert data.count(b"\xFF\x00") >= int((want == 0xFF).sum())
        # the restatement's byte-at-a-time walk agrees
        h, w, quant, specs, scan = D.split_file(data)
        assert (h, w) == (H, W) and np.array_equal(quant, p.quant) and tuple(specs) == p.specs and np.array_equal(scan, p.scan)
    if quality == 100:
        assert stuffed > 0                                                       # scans that hold FF bytes were among them


def test_parse_jpeg_on_a_scan_of_ff_bytes():
    """FF bytes back to back, at the scan's first and last byte"""
    stream = np.array([0xFF, 0xFF, 0x00, 0x12, 0xFF, 0x00, 0xFF], np.uint8)
    data = V.jpeg_header(16, 16, 90) + V.finish_scan(stream, 8 * len(stream))
    assert data.endswith(b"\xFF\x00\xFF\x00\x00\x12\xFF\x00\x00\xFF\x00\xFF\xD9")
    assert np.array_equal(V.parse_jpeg(data).scan, stream)
    assert np.array_equal(V.parse_jpeg(data[:-2]).scan, stream)                  # a file that lost its EOI
    assert len(V.parse_jpeg(V.jpeg_header(16, 16, 90) + b"\xFF\xD9").scan) == 0


def test_parse_jpeg_on_a_baseline_file_without_its_eoi():
    """a baseline scan that runs to the end of the data, no marker behind it, parses to the scan bytes of the whole file - with and
    without restart intervals - while a progressive scan cut like that stays refused"""
    from PIL import Image
    pic = D.picture(24, 40, 6)
    for kw in (dict(), dict(restart_marker_blocks=2)):
        buf = io.BytesIO()
        Image.fromarray(pic).save(buf, format="JPEG", quality=90, subsampling=2, **kw)
        data = buf.getvalue()
        assert data.endswith(b"\xFF\xD9")
        whole, cut = (V.parse_jpeg(d, restart=True) for d in (data, data[:-2]))
        assert len(whole.scan) > 0 and np.array_equal(cut.scan, whole.scan) and np.array_equal(cut.intervals, whole.intervals)
        assert cut.restart == whole.restart == (2 if kw else 0) and len(cut.intervals) - 1 == (3 if kw else 1)
    buf = io.BytesIO()
    Image.fromarray(pic).save(buf, format="JPEG", quality=90, progressive=True)
    data = buf.getvalue()
    assert len(V.parse_jpeg(data, progressive=True).scans) > 1
    with pytest.raises(ValueError, match="no marker"):
        V.parse_jpeg(data[:-2], progressive=True)


def test_parse_jpeg_fills_in_the_standard_tables_when_dht_is_absent():
    files, _ = framed_files("ramp", 1, 24, 40, 50)
    data, out, pos = files[0], [files[0][:2]], 2
    while data[pos + 1] != 0xDA:                               # drop the four DHT segments: what Motion-JPEG AVI writers do
        size = struct.unpack_from(">H", data, pos + 2)[0]
        if data[pos + 1] != 0xC4:
            out.append(data[pos:pos + 2 + size])
        pos += 2 + size
    bare = b"".join(out) + data[pos:]
    assert len(bare) < len(data) - 400 and b"\xFF\xC4" not in bare[:pos]
    p, q = V.parse_jpeg(bare), V.parse_jpeg(data)
    assert p.specs == tuple(V.HUFFMAN_SPECS) == q.specs and np.array_equal(p.scan, q.scan) and np.array_equal(p.quant, q.quant)


def pillow_save(frame, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def with_restart_interval(frame):
    """a file with a restart interval: Pillow's own where it takes restart_marker_blocks, otherwise a DRI segment spliced in"""
    data = pillow_save(frame, quality=90, subsampling=2, restart_marker_blocks=1)
    if b"\xFF\xDD\x00\x04" in data:
        return data
    plain = pillow_save(frame, quality=90, subsampling=2)
    at = plain.index(b"\xFF\xDA")
    return plain[:at] + b"\xFF\xDD\x00\x04\x00\x01" + plain[at:]


def test_parse_jpeg_refuses_what_is_not_built():
    frame = D.picture(40, 24, 1)
    assert V.parse_jpeg(pillow_save(frame, quality=90, subsampling=2)).width == 24
    for data, says in ((pillow_save(frame, quality=90, subsampling=2, progressive=True), "progressive"),
                       (pillow_save(frame, quality=90, subsampling=0), "1x1 / 1x1 / 1x1"),
                       (pillow_save(frame, quality=90, subsampling=1), "2x1 / 1x1 / 1x1"),
                       (pillow_save(frame[..., 0], quality=90), "grey"),
                       (with_restart_interval(frame), "restart"),
                       (pillow_save(frame[:, :4], quality=90, subsampling=2), "4 pixels wide"),
                       (b"RIFF....AVI ", "not a JPEG"),
                       (V.jpeg_header(16, 16, 90)[:100], "runs past the end of the file"),
                       (V.jpeg_header(16, 16, 90)[:89], "ends or is damaged")):
        with pytest.raises(ValueError, match=says):
            V.parse_jpeg(data)
    assert V.parse_jpeg(pillow_save(frame[:, :5], quality=90, subsampling=2)).width == 5
    # 16-bit quantisers, and Cb / Cr on different Huffman tables, spliced into a good file
    good = V.jpeg_header(16, 16, 90) + b"\xFF\xD9"
    at = good.index(b"\xFF\xDB")
    wide = good[:at] + b"\xFF\xDB" + struct.pack(">H", 2 + 1 + 128) + bytes([0x10]) + bytes(128) + good[at:]
    with pytest.raises(ValueError, match="16-bit"):
        V.parse_jpeg(wide)
    sos = good.index(b"\xFF\xDA")
    split = good[:sos + 4] + bytes([3, 1, 0x00, 2, 0x11, 3, 0x10, 0, 63, 0]) + good[sos + 14:]
    with pytest.raises(ValueError, match="Cb decodes with"):
        V.parse_jpeg(split)


def test_decode_mjpeg_refusals_that_need_no_device():
    with pytest.raises(ValueError, match="no frames"):
        V.decode_mjpeg([])
    with pytest.raises(V.ops._lib.EmoHipError, match="no host decoder"):
        V.decode_mjpeg([V.jpeg_header(16, 16, 90) + b"\xFF\xD9"], device="cpu")
