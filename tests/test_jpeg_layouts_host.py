"""Host tests of the JPEG layouts (no device): the numpy restatement of tests/jpeg_layout_ref.py against Pillow's decoder (libjpeg) byte
for byte - 4:4:4, 4:2:2, 4:2:0 and grey, over the sizes at which each part can go wrong, three qualities, standard and optimised Huffman
tables, three quantisers - and emote_hack_amd.video_io.parse_jpeg(layouts=True): the layout, the table selectors and the MCU count it
returns, and what it refuses by name."""
import struct

import numpy as np
import pytest

from emote_hack_amd import video_io as V
from tests import jpeg_decode_ref as D
from tests import jpeg_layout_ref as L

CASES = [(name, H, W) for name in L.LAYOUTS for H, W in L.SIZES[name]]


@pytest.mark.parametrize("name,H,W", CASES)
def test_restatement_equals_pillow(name, H, W):
    for quality in L.QUALITIES:
        for optimize in (False, True):
            data = L.pillow_file(D.picture(H, W, H * W + quality), name, quality, optimize)
            f, coefs, y, c, rgb = L.decode_all(data)
            assert f["layout"] == L.LAYOUTS[name] and coefs.shape[1] == L.bpm(f["layout"])
            assert np.array_equal(rgb, L.pillow_decode(data)), (name, H, W, quality, optimize)


def test_restatement_equals_pillow_on_three_quantisers_and_restart_intervals():
    pic = D.picture(17, 33, 3)
    for name in ("4:4:4", "4:2:2", "4:2:0"):
        data = L.three_quantiser_file(pic, name)
        f = L.split_file(data)
        assert f["tq"] == (0, 1, 2) and not np.array_equal(f["quant"][1], f["quant"][2])
        assert np.array_equal(L.decode(data), L.pillow_decode(data)), name
    for name in L.LAYOUTS:
        for kw in (dict(restart_marker_blocks=1), dict(restart_marker_blocks=2), dict(restart_marker_rows=1)):
            data = L.pillow_file(pic, name, 90, False, **kw)
            assert len(L.split_file(data)["parts"]) > 1
            assert np.array_equal(L.decode(data), L.pillow_decode(data)), (name, kw)


@pytest.mark.parametrize("name", list(L.LAYOUTS))
def test_parse_jpeg_returns_the_layout(name):
    H, W = 38, 70
    for optimize in (False, True):
        data = L.pillow_file(D.picture(H, W, 7), name, 90, optimize)
        p, f = V.parse_jpeg(data, layouts=True), L.split_file(data)
        nc, hs, vs = L.LAYOUTS[name]
        assert (p.height, p.width) == (H, W) and p.layout.key == (nc, hs, vs) and p.layout.name == name and p.layout.components == nc
        assert p.layout.factors == (((hs, vs), (1, 1), (1, 1)) if nc == 3 else ((1, 1),))
        assert p.layout.blocks_per_mcu == L.bpm(L.LAYOUTS[name]) == {"4:4:4": 3, "4:2:2": 4, "4:2:0": 6, "grey": 1}[name]
        mr, mc = L.grid(H, W, L.LAYOUTS[name])
        assert p.mcus == mr * mc == V.ops.jpeg_mcus(H, W, p.layout.key) == {"4:4:4": 45, "4:2:2": 25, "4:2:0": 15, "grey": 45}[name]
        assert p.layout.quant == f["tq"] == ((0, 1, 1) if nc == 3 else (0,))
        assert p.layout.huffman == f["tables"] == (((0, 0), (1, 1), (1, 1)) if nc == 3 else ((0, 0),))
        assert p.quants.dtype == np.uint16 and np.array_equal(p.quants, f["quant"]) and np.array_equal(p.quant, f["quant"][:2])
        assert list(p.specs) == f["specs"] and np.array_equal(p.scan, f["parts"][0]) and p.restart == 0
        assert (p.layout.key == (3, 2, 2) and np.array_equal(p.quants[1], p.quants[2])) == (name == "4:2:0")
    assert V.ops.jpeg_mcus(H, W) == V.ops.jpeg_mcus(H, W, (3, 2, 2)) == 15       # jpeg_mcus keeps its meaning: 4:2:0 unless told


def test_parse_jpeg_on_three_quantisers_and_a_restart_file():
    pic = D.picture(17, 33, 3)
    data = L.three_quantiser_file(pic)
    p, f = V.parse_jpeg(data, layouts=True), L.split_file(data)
    assert p.layout.name == "4:4:4" and p.layout.quant == (0, 1, 2) and np.array_equal(p.quants, f["quant"]) and p.layout.key != (3, 2, 2)
    assert len({p.quants[k].tobytes() for k in range(3)}) == 3
    with pytest.raises(ValueError, match="Cb and Cr use different quantisation tables"):
        V.parse_jpeg(L.three_quantiser_file(pic, "4:2:0"))                       # without the keyword: as before
    p420 = V.parse_jpeg(L.three_quantiser_file(pic, "4:2:0"), layouts=True)
    assert p420.layout.name == "4:2:0" and p420.layout.key == (3, 2, 2) and not np.array_equal(p420.quants[1], p420.quants[2])
    assert p420.layout.quant == (0, 1, 2)
    # 33 x 17 at 4:2:2: MCUs of 16 x 8, 3 x 3 = 9 of them; a restart interval of 2 makes 5 intervals, the last of one MCU
    data = L.pillow_file(pic, "4:2:2", 90, False, restart_marker_blocks=2)
    p, f = V.parse_jpeg(data, restart=True, layouts=True), L.split_file(data)
    assert p.layout.name == "4:2:2" and p.mcus == 9 and p.restart == 2 == f["ri"] and len(p.intervals) - 1 == 5 == len(f["parts"])
    for k, part in enumerate(f["parts"]):
        assert np.array_equal(p.scan[p.intervals[k]:p.intervals[k + 1]], part)
    # grey restart intervals count in blocks: 5 x 3 = 15 blocks, a row of 5 per interval
    data = L.pillow_file(pic, "grey", 90, False, restart_marker_rows=1)
    p = V.parse_jpeg(data, restart=True, layouts=True)
    assert p.mcus == 15 and p.restart == 5 and len(p.intervals) - 1 == 3
    with pytest.raises(ValueError, match="restart"):
        V.parse_jpeg(data, layouts=True)


def patched(data, at, new):
    return data[:at] + bytes(new) + data[at + len(bytes(new)):]


def test_parse_jpeg_refusals_name_what_was_found():
    pic = D.picture(16, 24, 1)
    good = L.pillow_file(pic, "4:2:2", 90, False)
    sof = good.index(b"\xFF\xC0")
    assert good[sof + 11] == 0x21                                                # the first component's sampling byte
    for byte, says in ((0x12, r"1x2 / 1x1 / 1x1 \(4:4:0\)"), (0x41, r"4x1 / 1x1 / 1x1 \(4:1:1\)"), (0x31, "3x1 / 1x1 / 1x1")):
        with pytest.raises(ValueError, match="sampling factors " + says):
            V.parse_jpeg(patched(good, sof + 11, [byte]), layouts=True)
    with pytest.raises(ValueError, match="2x1 / 2x1 / 1x1"):                     # chrominance is 1x1 in every layout that is built
        V.parse_jpeg(patched(good, sof + 14, [0x21]), layouts=True)
    # four components: the SOF0 segment rewritten with a fourth
    body = good[sof + 4:sof + 4 + 15]
    four = good[:sof] + b"\xFF\xC0" + struct.pack(">H", 2 + 6 + 12) + body[:5] + bytes([4]) + body[6:] + bytes([4, 0x11, 1]) + good[sof + 19:]
    with pytest.raises(ValueError, match="4 components"):
        V.parse_jpeg(four, layouts=True)
    # colour spaces libjpeg reads as RGB: Adobe transform 0; no JFIF, no Adobe and ids R, G, B
    adobe = lambda transform: b"\xFF\xEE" + struct.pack(">H", 14) + b"Adobe" + struct.pack(">HHHB", 100, 0, 0, transform)
    with pytest.raises(ValueError, match="Adobe APP14 segment with transform 0"):
        V.parse_jpeg(good[:sof] + adobe(0) + good[sof:], layouts=True)
    plain = L.pillow_file(pic, "4:2:0", 90, False)                               # and with or without the keyword on a 4:2:0 file
    for kw in (dict(), dict(layouts=True)):
        with pytest.raises(ValueError, match="Adobe APP14 segment with transform 0"):
            V.parse_jpeg(plain[:plain.index(b"\xFF\xC0")] + adobe(0) + plain[plain.index(b"\xFF\xC0"):], **kw)
    assert V.parse_jpeg(good[:sof] + adobe(1) + good[sof:], layouts=True).layout.name == "4:2:2"      # transform 1 is YCbCr
    app0 = good.index(b"\xFF\xE0")
    size = struct.unpack_from(">H", good, app0 + 2)[0]
    assert good[app0 + 4:app0 + 9] == b"JFIF\0"
    bare = good[:app0] + good[app0 + 2 + size:]
    assert V.parse_jpeg(bare, layouts=True).layout.name == "4:2:2"               # ids 1, 2, 3 without JFIF: still YCbCr
    at, sos = bare.index(b"\xFF\xC0"), bare.index(b"\xFF\xDA")
    rgb = bytearray(bare)
    for i, cid in enumerate(b"RGB"):
        rgb[at + 10 + 3 * i] = rgb[sos + 5 + 2 * i] = cid
    with pytest.raises(ValueError, match="component ids 'R', 'G', 'B'"):
        V.parse_jpeg(bytes(rgb), layouts=True)
    jfif_rgb = bytes(rgb[:app0]) + good[app0:app0 + 2 + size] + bytes(rgb[app0:])
    assert V.parse_jpeg(jfif_rgb, layouts=True).layout.name == "4:2:2"           # JFIF implies YCbCr whatever the ids
    # everything the parser refused before is still refused under the keyword
    from PIL import Image
    import io
    buf = io.BytesIO()
    Image.fromarray(pic).save(buf, format="JPEG", quality=90, subsampling=1, progressive=True)
    with pytest.raises(ValueError, match="progressive"):
        V.parse_jpeg(buf.getvalue(), layouts=True)
    sos = good.index(b"\xFF\xDA")
    split = good[:sos + 4] + bytes([3, 1, 0x00, 2, 0x11, 3, 0x10, 0, 63, 0]) + good[sos + 14:]
    with pytest.raises(ValueError, match="Cb decodes with"):
        V.parse_jpeg(split, layouts=True)


def test_width_limit_holds_where_chroma_is_halved_along_the_rows():
    pic = D.picture(9, 4, 2)
    for name in ("4:2:2", "4:2:0"):
        with pytest.raises(ValueError, match="4 pixels wide"):
            V.parse_jpeg(L.pillow_file(pic, name, 90, False), layouts=True)
        assert V.parse_jpeg(L.pillow_file(D.picture(9, 5, 2), name, 90, False), layouts=True).width == 5
    for name in ("4:4:4", "grey"):
        for w in (4, 1):
            assert V.parse_jpeg(L.pillow_file(pic[:, :w], name, 90, False), layouts=True).width == w


def test_without_the_keyword_parse_jpeg_takes_what_it_took():
    pic = D.picture(16, 24, 1)
    for name, says in (("4:4:4", "1x1 / 1x1 / 1x1"), ("4:2:2", "2x1 / 1x1 / 1x1"), ("grey", "grey")):
        with pytest.raises(ValueError, match=says):
            V.parse_jpeg(L.pillow_file(pic, name, 90, False))
    p = V.parse_jpeg(L.pillow_file(pic, "4:2:0", 90, False))
    assert p.layout.key == (3, 2, 2) and np.array_equal(p.quants[1], p.quants[2]) and p.mcus == V.ops.jpeg_mcus(16, 24)
