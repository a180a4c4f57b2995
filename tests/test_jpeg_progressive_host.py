"""CPU tests of the progressive JPEG path's host half and of its yardstick: tests/jpeg_progressive_ref.py's decoder (plus the IDCT and
colour restatements of tests/jpeg_layout_ref.py) against Pillow byte for byte - on Pillow's own progressive files and on every file the
script writer makes, which Pillow must open without a warning - and parse_jpeg(progressive=True): the scan records, the restart interval
that changes from scan to scan, every refusal, and baseline files parsing to what they parse to without the keyword.

test_reference_decoder_equals_pillow_on_pillow_files and test_reference_decoder_on_the_flat_frame_with_long_eob_runs run no product code:
they pin the yardstick - the reference decoder of tests/jpeg_progressive_ref.py against Pillow - that the GPU tests hold the kernel to,
so they pass with or without the feature and are no coverage of it."""
import functools
import io
import struct
import warnings

import numpy as np
import pytest

from emote_hack_amd import video_io as V
from tests import jpeg_decode_ref as D
from tests import jpeg_layout_ref as L
from tests import jpeg_progressive_ref as P

RESTARTS = [dict(restart_marker_rows=1), dict(restart_marker_blocks=1)]
SCRIPT_SIZES = [(9, 17), (38, 70)]


def pillow_strict(data):
    """Pillow's decode with every warning an error: libjpeg's "corrupt data" and "bogus progression" messages arrive as warnings"""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return L.pillow_decode(data)


@functools.lru_cache(maxsize=None)
def written(name, H, W, script, restart=True):
    """(a file the writer makes from the coefficients of Pillow's baseline file of a picture, that baseline file)"""
    base = L.pillow_file(D.picture(H, W, H * W + 7), name, 90, False)
    f = L.split_file(base)
    return P.write_progressive(L.coefficients(f), f["quant"], H, W, L.LAYOUTS[name], P.scripts(L.LAYOUTS[name][0], restart)[script]), base


@pytest.mark.parametrize("name", list(L.LAYOUTS))
def test_reference_decoder_equals_pillow_on_pillow_files(name):
    for H, W in P.SIZES:
        for quality in P.QUALITIES:
            pic = D.picture(H, W, H * W + quality)
            data = P.pillow_progressive(pic, name, quality)
            want = pillow_strict(data)
            assert np.array_equal(P.decode(data), want), (H, W, quality)
            # a complete progressive file decodes to the bytes of the baseline file: no inter-block smoothing runs
            assert np.array_equal(want, L.pillow_decode(L.pillow_file(pic, name, quality, False))), (H, W, quality)
        for kw in RESTARTS:
            data = P.pillow_progressive(D.picture(H, W, H * W + 90), name, 90, **kw)
            assert np.array_equal(P.decode(data), pillow_strict(data)), (H, W, kw)


def test_reference_decoder_on_the_flat_frame_with_long_eob_runs():
    data = P.pillow_progressive(P.flat_picture(), "4:4:4", 90)
    f = P.split_progressive(data)
    assert np.array_equal(P.decode(data), pillow_strict(data))
    # one AC scan of 272 blocks in a single EOB run: an EOB8 symbol (0x80) and its 8 extra bits
    ac = [sc for sc in f["scans"] if sc["Ss"] > 0 and sc["Ah"] == 0]
    assert ac and all(len(sc["parts"]) == 1 and len(sc["parts"][0]) <= 4 for sc in ac)
    assert P.units_of(*P.FLAT, (3, 1, 1), (0,)) == 272


@pytest.mark.parametrize("name", list(L.LAYOUTS))
def test_written_scripts_open_in_pillow_and_decode_to_the_baseline_bytes(name):
    for H, W in SCRIPT_SIZES:
        for script in P.scripts(L.LAYOUTS[name][0]):
            data, base = written(name, H, W, script)
            want = pillow_strict(data)
            assert np.array_equal(want, L.pillow_decode(base)), (H, W, script)
            assert np.array_equal(P.decode(data), want), (H, W, script)
            p = V.parse_jpeg(data, progressive=True)
            assert [(s.components, s.Ss, s.Se, s.Ah, s.Al) for s in p.scans] == \
                [(sc["comps"], sc["Ss"], sc["Se"], sc["Ah"], sc["Al"]) for sc in P.scripts(L.LAYOUTS[name][0])[script]]
        plain, _ = written(name, H, W, "restart", False)
        assert np.array_equal(pillow_strict(plain), L.pillow_decode(base))
        with_ri, without = V.parse_jpeg(written(name, H, W, "restart")[0], progressive=True), V.parse_jpeg(plain, progressive=True)
        assert [s.restart for s in with_ri.scans] == [3, 0, 3, 3, 0, 3, 0][:len(with_ri.scans)] and not any(s.restart for s in without.scans)
        assert any(len(s.intervals) > 2 for s in with_ri.scans)


def test_four_destinations_script_reaches_the_parser_with_the_tables_of_each_scan():
    data, _ = written("4:2:0", 38, 70, "four destinations")
    p = V.parse_jpeg(data, progressive=True)
    assert p.scans[0].huffman == ((3, 0), (1, 1), (2, 2)) and [s[0] for s in p.scans[0].specs] == [P.TABLES[t] for t in ("dcB", "dcB", "dcC")]
    cb, cr = (next(s for s in p.scans if s.components == (c,) and s.Ss == 1) for c in (1, 2))
    assert cb.specs[0][1] == P.TABLES["acB"] and cr.specs[0][1] == P.TABLES["acC"]
    # destination (AC, 1) is acB for Cb's scan and acC, redefined by a DHT between scans, for the luminance band 21 .. 63
    late = next(s for s in p.scans if s.Ss == 21)
    assert late.huffman == ((3, 1),) and late.specs[0][1] == P.TABLES["acC"] and late.specs[0][0] == P.TABLES["dcB"]


# ------------------------------------------------------------------------------------------------------------------- parse_jpeg
def test_scan_records_of_a_pillow_file():
    H, W = 9, 17
    pic = D.picture(H, W, 5)
    data = P.pillow_progressive(pic, "4:2:0", 90)
    p = V.parse_jpeg(data, progressive=True)
    f = P.split_progressive(data)
    assert (p.height, p.width, p.layout.key, p.restart) == (H, W, (3, 2, 2), 0) and np.array_equal(p.quants[1], p.quants[2]) and len(p.scans) == 10 == len(f["scans"])
    assert np.array_equal(p.quants, f["quant"]) and p.specs == () and len(p.scan) == 0
    # libjpeg's default script (jcparam.c jpeg_simple_progression)
    assert [s.script for s in p.scans] == [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
                                           ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
    for s, sc in zip(p.scans, f["scans"]):
        assert s.huffman == sc["tables"] and s.restart == 0 and len(s.intervals) == 2
        assert np.array_equal(s.scan, sc["parts"][0])
        for (dc, ac), (td, ta) in zip(s.specs, sc["tables"]):                    # the tables as the DHT segments in front of THIS scan left them
            assert dc == sc["huff"].get((0, td)) and ac == sc["huff"].get((1, ta))
    grey = V.parse_jpeg(P.pillow_progressive(pic, "grey", 90), progressive=True)
    assert len(grey.scans) == 6 and grey.layout.key == (1, 1, 1) and all(s.components == (0,) for s in grey.scans)
    # Pillow optimises the tables per scan: one destination holds different tables at different scans
    assert len({s.specs[0][1] for s in p.scans if s.components == (0,)}) > 1


def test_restart_interval_changes_from_scan_to_scan():
    data = P.pillow_progressive(D.picture(9, 17, 5), "4:2:0", 90, restart_marker_rows=1)
    p = V.parse_jpeg(data, progressive=True)
    # a row of MCUs in the interleaved scans (2), a row of blocks in the one-component ones: 3 for luminance, 2 for chrominance
    assert [s.restart for s in p.scans] == [2, 3, 2, 2, 3, 3, 2, 2, 2, 3] and p.restart == 2
    assert [len(s.intervals) - 1 for s in p.scans] == [1, 2, 1, 1, 2, 2, 1, 1, 1, 2]
    f = P.split_progressive(data)
    for s, sc in zip(p.scans, f["scans"]):
        assert s.restart == sc["ri"] and len(s.intervals) - 1 == len(sc["parts"])
        for k, part in enumerate(sc["parts"]):
            assert np.array_equal(s.scan[s.intervals[k]:s.intervals[k + 1]], part)
    blocks = V.parse_jpeg(P.pillow_progressive(D.picture(38, 70, 5), "4:2:2", 90, restart_marker_blocks=1), progressive=True)
    assert all(s.restart == 1 for s in blocks.scans) and len(blocks.scans[1].intervals) - 1 == 5 * 9


def test_baseline_files_parse_as_without_the_keyword():
    pic = D.picture(38, 70, 3)
    for name in L.LAYOUTS:
        for kw in (dict(), dict(restart_marker_rows=1)):
            data = L.pillow_file(pic, name, 90, True, **kw)
            a, b = V.parse_jpeg(data, restart=True, layouts=True), V.parse_jpeg(data, progressive=True)
            assert b.scans is None and a.scans is None
            assert (a.height, a.width, a.specs, a.restart, a.layout) == (b.height, b.width, b.specs, b.restart, b.layout)
            assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("quant", "quants", "scan", "intervals"))
            assert a.table_key() == b.table_key()
    with pytest.raises(ValueError, match="a progressive \\(SOF2\\) file"):
        V.parse_jpeg(P.pillow_progressive(pic, "4:2:0", 90), restart=True, layouts=True)


def _scan_headers(data):
    """byte positions of the SOS markers of a file whose entropy-coded bytes cannot hold FF DA (stuffing) - the tables in front could,
    so the walk goes marker by marker"""
    pos, out = 2, []
    while data[pos + 1] != 0xD9:
        size = struct.unpack_from(">H", data, pos + 2)[0]
        if data[pos + 1] == 0xDA:
            out.append(pos)
            pos += 2 + size
            while not (data[pos] == 0xFF and data[pos + 1] not in (0x00,) and not 0xD0 <= data[pos + 1] <= 0xD7):
                pos += 1
        else:
            pos += 2 + size
    return out, pos


def _with_sos(data, at, **fields):
    """the file with fields of the SOS header at `at` replaced: Ss, Se, AhAl, or comps=[(id, tables byte), ...]"""
    ns = data[at + 4]
    head = bytearray(data[at:at + 4 + 1 + 2 * ns + 3])
    comps = fields.get("comps")
    if comps is not None:
        tail = bytes(head[5 + 2 * ns:])
        head = bytearray(b"\xFF\xDA" + struct.pack(">H", 6 + 2 * len(comps)) + bytes([len(comps)]) + b"".join(bytes(c) for c in comps) + tail)
        ns_new = len(comps)
    else:
        ns_new = ns
    for key, off in (("Ss", 0), ("Se", 1), ("AhAl", 2)):
        if key in fields:
            head[5 + 2 * ns_new + off] = fields[key]
    return data[:at] + bytes(head) + data[at + 4 + 1 + 2 * ns + 3:]


def test_refusals():
    pic = D.picture(38, 70, 3)
    good = P.pillow_progressive(pic, "4:2:0", 90)
    sos, eoi = _scan_headers(good)
    assert len(sos) == 10 and good[eoi:] == b"\xFF\xD9"

    def refused(data, says):
        with pytest.raises(ValueError, match=says):
            V.parse_jpeg(data, progressive=True)
    refused(_with_sos(good, sos[0], Se=5), "starts at the DC coefficient holds it alone")
    refused(_with_sos(good, sos[1], comps=[(1, 0x00), (2, 0x11)]), "an AC scan interleaved over 2 components")
    refused(_with_sos(good, sos[1], Ss=6, Se=5), "an AC band runs from Ss up to Se <= 63")
    refused(_with_sos(good, sos[1], Se=64), "an AC band runs from Ss up to Se <= 63")
    refused(_with_sos(good, sos[1], AhAl=0x0E), "Al above 13")
    refused(_with_sos(good, sos[1], AhAl=0x32), "the first scan of coefficient 1 of component 1 with Ah = 3, not 0")
    refused(_with_sos(good, sos[5], AhAl=0x10), "a refinement of coefficient 1 of component 1 with Ah = 1, the scan before it left Al = 2")
    refused(_with_sos(good, sos[5], AhAl=0x22), "a refinement steps down by one bit")
    refused(_with_sos(good, sos[5], AhAl=0x01), "with Ah = 0, the scan before it left Al = 2")
    refused(_with_sos(good, sos[1], comps=[(7, 0x00)]), "names component 7, the frame has \\[1, 2, 3\\]")
    refused(_with_sos(good, sos[0], comps=[(1, 0x00), (2, 0x11)]), "interleaved over 2 of the frame's 3 components")
    refused(_with_sos(good, sos[0], comps=[(2, 0x10), (1, 0x00), (3, 0x10)]), "lists its components out of the frame's order")
    sof = good.index(b"\xFF\xC2")
    refused(good[:sof + 4] + good[sof + 5:], "a malformed SOF2 segment")
    # an AC scan of a component in front of its first DC scan: the first scan made a DC scan of luminance alone
    refused(_with_sos(good, sos[0], comps=[(1, 0x00)]), "an AC scan of component 3 in front of that component's first DC scan")
    # a progression that stops early: cut after the sixth scan, EOI put back.  Pillow opens it; libjpeg smooths it
    cut = good[:sos[6]] + b"\xFF\xD9"
    assert L.pillow_decode(cut).shape == (38, 70, 3)
    refused(cut, "the progression is not complete at EOI after 6 scans: coefficient 0 of component 1 coded down to Al = 1 only, not to 0.*smooths")
    refused(good[:sos[2]] + b"\xFF\xD9", "not complete at EOI after 2 scans: coefficients 6 .. 63 of component 1 never coded.*jdcoefct.c smoothing_ok")
    refused(good[:sos[6] - 1], "runs to the end of the file|no marker at byte")
    # a DQT behind the first SOS that changes a table in use; the same table again is harmless
    dqt = good.index(b"\xFF\xDB")
    size = struct.unpack_from(">H", good, dqt + 2)[0]
    seg = bytearray(good[dqt:dqt + 2 + size])
    assert V.parse_jpeg(good[:sos[3]] + bytes(seg) + good[sos[3]:], progressive=True).scans is not None
    seg[5 + 10] ^= 1
    refused(good[:sos[3]] + bytes(seg) + good[sos[3]:], "a DQT segment behind scan 2 changes quantisation table 0")
    refused(good[:sos[3]] + b"\xFF\xDC\x00\x04\x00\x26" + good[sos[3]:], "a DNL segment behind scan 2")
    # arithmetic-coded progressive and the other frame types, as before
    sof = good.index(b"\xFF\xC2")
    for marker, says in ((0xCA, "arithmetic-coded progressive \\(SOF10\\)"), (0xC1, "extended sequential \\(SOF1\\)"), (0xC6, "differential progressive")):
        refused(good[:sof + 1] + bytes([marker]) + good[sof + 2:], says)
    # everything baseline is refused for: sampling factors, 16-bit quantisers, RGB, the width limit
    bad = bytearray(good)
    bad[sof + 11] = 0x12
    refused(bytes(bad), "sampling factors 1x2 / 1x1 / 1x1 \\(4:4:0\\)")
    bad = bytearray(good)
    bad[sof + 11] = 0x41
    refused(bytes(bad), "\\(4:1:1\\)")
    bad = bytearray(good)
    bad[dqt + 4] |= 0x10
    refused(bytes(bad), "16-bit entries")
    adobe = b"\xFF\xEE" + struct.pack(">H", 14) + b"Adobe" + struct.pack(">HHHB", 100, 0, 0, 0)
    refused(good[:sof] + adobe + good[sof:], "Adobe APP14 segment with transform 0")
    for name in ("4:2:0", "4:2:2"):
        refused(P.pillow_progressive(D.picture(9, 4, 2), name, 90), "4 pixels wide")
    assert V.parse_jpeg(P.pillow_progressive(D.picture(9, 4, 2), "4:4:4", 90), progressive=True).width == 4
    # Cb and Cr on different Huffman tables stay refused for baseline files, and are fine in progressive scans
    base = L.pillow_file(pic, "4:2:2", 90, False)
    at = base.index(b"\xFF\xDA")
    refused(base[:at + 4] + bytes([3, 1, 0x00, 2, 0x11, 3, 0x10, 0, 63, 0]) + base[at + 14:], "Cb decodes with")
    assert V.parse_jpeg(_with_sos(good, sos[0], comps=[(1, 0x00), (2, 0x10), (3, 0x00)]), progressive=True).scans[0].huffman == ((0, 0), (1, 0), (0, 0))
    # restart markers must still cut a scan into the intervals its own DRI and unit count make
    ri = P.pillow_progressive(pic, "4:2:0", 90, restart_marker_rows=1)
    last = ri.index(b"\xFF\xD1", _scan_headers(ri)[0][0])                         # three rows of MCUs: RST0, RST1
    refused(ri[:last] + ri[last + 2:], "2 restart intervals in scan 0 .*15 units at a restart interval of 5 make 3")
    first = ri.index(b"\xFF\xD0", _scan_headers(ri)[0][0])
    refused(ri[:first] + ri[first + 2:], "restart marker 0 of scan 0 .* is RST1")


def test_decode_mjpeg_keyword_is_checked_before_any_launch():
    """the device is asked for before any file is read, with and without the keyword"""
    from emote_hack_amd import _lib
    with pytest.raises(_lib.EmoHipError, match="decodes on the HIP device"):
        V.decode_mjpeg([P.pillow_progressive(D.picture(8, 8, 1), "4:2:0", 90)], device="cpu", progressive=True)
