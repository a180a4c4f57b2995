"""CPU tests of JPEG restart intervals (T.81 B.2.4.4, E.1.4): tests/jpeg_restart_ref.py against Pillow's encoder and decoder byte for byte,
parse_jpeg(restart=True) against the reference's own walk, what it refuses, the host half of the writer (padding, stuffing, marker
numbering) and the validation of restart_interval=.  Everything is an equality."""
import struct

import numpy as np
import pytest

from emote_hack_amd import video_io as V
from tests import jpeg_decode_ref as D
from tests import jpeg_restart_ref as RR
from tests import mjpeg_ref as R

SIZES = [(16, 16), (24, 40), (70, 38), (64, 64)]         # (H, W): 1, 6, 15 and 16 MCUs


def frame_of(H, W):
    return R.make_frames("noise", 1, H, W)[0] if (H, W) == (64, 64) else D.picture(H, W, H * W)


def pillow_settings(H, W):
    n_mcu = int(np.prod(R.n_mcus(H, W)))
    return [dict(blocks=1), dict(blocks=4), dict(blocks=n_mcu), dict(blocks=n_mcu + 5), dict(rows=1)]


def expected_ri(kw, H, W):
    return kw["blocks"] if "blocks" in kw else R.n_mcus(H, W)[1] * kw["rows"]


# ------------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("H,W", SIZES)
def test_reference_equals_pillow(H, W):
    frame = frame_of(H, W)
    n_mcu = int(np.prod(R.n_mcus(H, W)))
    for quality in RR.QUALITIES:
        plain = R.decode(D.pillow_file(frame, quality, False))
        for kw in pillow_settings(H, W):
            data = RR.pillow_restart_file(frame, quality, **kw)
            _, _, _, _, ri, parts, markers = RR.split_restart_file(data)
            assert ri == expected_ri(kw, H, W) and len(parts) == RR.n_intervals(n_mcu, ri), (H, W, quality, kw)
            assert markers == [k % 8 for k in range(len(parts) - 1)]             # they cycle mod 8, none behind the last interval
            want = R.decode(data)
            assert np.array_equal(RR.decode(data), want), (H, W, quality, kw)    # interval by interval = Pillow's decoder
            assert np.array_equal(want, plain), (H, W, quality, kw)              # and the intervals do not change the picture
    if (H, W) == (64, 64):       # the long segment of the GPU tests: one interval of more than a 4 KiB window
        parts = RR.split_restart_file(RR.pillow_restart_file(frame, 100, blocks=n_mcu))[5]
        assert len(parts) == 1 and len(parts[0]) > 4096, len(parts[0])


def test_interval_encoding_restarts_the_predictions():
    """entropy_intervals is mjpeg_ref.entropy per interval: with one interval it is the frame's stream, with more every interval decodes
    on its own to the coefficients it was given"""
    t = V.jpeg_tables(90)
    coefs, _ = R.blocks(R.make_frames("ramp", 2, 70, 38), t.quant)
    counts, streams = RR.entropy_intervals(coefs, t.huff, 15)
    c0, s0, _ = R.entropy(coefs, t.huff)
    assert np.array_equal(counts, c0) and all(len(s) == 1 and np.array_equal(s[0][0], w[0]) and s[0][1] == w[1] for s, w in zip(streams, s0))
    counts, streams = RR.entropy_intervals(coefs, t.huff, 4)
    assert not np.array_equal(counts, c0) and [len(s) for s in streams] == [4, 4]
    for f in range(2):
        parts = [s[:(b + 7) // 8] for s, b in streams[f]]
        assert np.array_equal(RR.decode_intervals(parts, t.specs, 15, 4), coefs[f])
        assert [b for _, b in streams[f]] == [int(counts[f, m0 * 6:m1 * 6].sum()) for m0, m1 in RR.interval_mcus(15, 4)]


# ------------------------------------------------------------------------------------------------------------------- the parser
@pytest.mark.parametrize("H,W", SIZES)
def test_parse_jpeg_gives_the_reference_intervals(H, W):
    frame = frame_of(H, W)
    for quality in RR.QUALITIES:
        for kw in pillow_settings(H, W):
            for optimize in (False, True):
                data = RR.pillow_restart_file(frame, quality, optimize=optimize, **kw)
                h, w, quant, specs, ri, parts, _ = RR.split_restart_file(data)
                p = V.parse_jpeg(data, restart=True)
                assert (p.height, p.width, p.restart) == (h, w, ri) and np.array_equal(p.quant, quant) and list(p.specs) == list(specs)
                assert len(p.intervals) == len(parts) + 1 and p.intervals[0] == 0 and p.intervals[-1] == len(p.scan)
                for k, part in enumerate(parts):
                    assert np.array_equal(p.scan[p.intervals[k]:p.intervals[k + 1]], part), (H, W, quality, kw, k)
    # a file without restart intervals: one interval, the whole scan, with the keyword and without
    plain = D.pillow_file(frame, 90, False)
    for p in (V.parse_jpeg(plain), V.parse_jpeg(plain, restart=True)):
        assert p.restart == 0 and list(p.intervals) == [0, len(p.scan)] and np.array_equal(p.scan, D.split_file(plain)[4])


def test_parse_jpeg_without_the_keyword_still_refuses():
    frame = D.picture(24, 40, 3)
    for kw in (dict(blocks=1), dict(blocks=11), dict(rows=1)):
        with pytest.raises(ValueError, match="restart markers are not built"):
            V.parse_jpeg(RR.pillow_restart_file(frame, 90, **kw))
    # markers in the scan of a file that defines no interval
    data = RR.pillow_restart_file(frame, 90, blocks=2)
    at = data.index(b"\xFF\xDD")
    no_dri = data[:at] + data[at + 6:]
    with pytest.raises(ValueError, match="a restart marker inside the scan; restart markers are not built"):
        V.parse_jpeg(no_dri)
    with pytest.raises(ValueError, match="2 restart markers in the scan .* no restart interval defined"):
        V.parse_jpeg(no_dri, restart=True)


def _markers(data):
    """positions of the RSTm markers in the scan of a file"""
    start = data.index(b"\xFF\xDA")
    return [i for i in range(start, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]


def test_parse_jpeg_refusals_under_the_keyword():
    frame = D.picture(24, 40, 3)                                                 # 6 MCUs
    data = RR.pillow_restart_file(frame, 90, blocks=1)
    m = _markers(data)
    assert len(m) == 5
    # markers out of order
    swapped = bytearray(data)
    swapped[m[1] + 1], swapped[m[2] + 1] = swapped[m[2] + 1], swapped[m[1] + 1]
    with pytest.raises(ValueError, match="restart marker 1 of the scan is RST2 .* RST1 is expected"):
        V.parse_jpeg(bytes(swapped), restart=True)
    # one interval too few: the last marker and interval cut away
    short = data[:m[-1]] + b"\xFF\xD9"
    with pytest.raises(ValueError, match="5 restart intervals in the scan, 6 MCUs at a restart interval of 1 make 6"):
        V.parse_jpeg(short, restart=True)
    # one too many: another marker and interval in front of EOI
    end = data.rindex(b"\xFF\xD9")
    long = data[:end] + b"\xFF\xD5" + data[m[-1] + 2:end] + b"\xFF\xD9"
    with pytest.raises(ValueError, match="7 restart intervals in the scan, 6 MCUs at a restart interval of 1 make 6"):
        V.parse_jpeg(long, restart=True)
    # an interval defined and no marker at all where several are due
    with pytest.raises(ValueError, match="1 restart interval in the scan"):
        V.parse_jpeg(data[:m[0]] + b"\xFF\xD9", restart=True)
    # a DRI segment of 4 bytes
    at = data.index(b"\xFF\xDD")
    assert data[at + 2:at + 4] == b"\x00\x04"
    fat = data[:at] + b"\xFF\xDD\x00\x06\x00\x00\x00\x01" + data[at + 6:]
    for kw in ({}, dict(restart=True)):
        with pytest.raises(ValueError, match="malformed DRI"):
            V.parse_jpeg(fat, **kw)
    # the last DRI in front of the scan holds; 0 takes the interval back
    twice = data[:at] + b"\xFF\xDD\x00\x04\x00\x07" + data[at:]
    assert V.parse_jpeg(twice, restart=True).restart == 1
    off = data[:at + 6] + b"\xFF\xDD\x00\x04\x00\x00" + data[at + 6:]
    with pytest.raises(ValueError, match="no restart interval defined"):
        V.parse_jpeg(off, restart=True)
    plain = D.pillow_file(frame, 90, False)
    sos = plain.index(b"\xFF\xDA")
    zero = V.parse_jpeg(plain[:sos] + b"\xFF\xDD\x00\x04\x00\x00" + plain[sos:])  # DRI 0 was never refused
    assert zero.restart == 0 and np.array_equal(zero.scan, V.parse_jpeg(plain).scan)


# ------------------------------------------------------------------------------------------------------------------- the writer's host half
def _bits(text):
    """"1011 0" -> (uint8 array with zero bits behind the last, number of bits)"""
    b = [int(c) for c in text if c in "01"]
    return np.packbits(np.array(b + [0] * (-len(b) % 8), np.uint8)), len(b)


def test_finish_restart_scan():
    parts = [_bits("10110"),                       # padded with three 1-bits
             _bits("11111111 0101"),               # an FF inside an interval
             _bits("00000001 11111111"),           # an FF that is the interval's last byte: 00 first, the marker behind it
             _bits("11111"),                       # 5 bits that padding turns into FF
             _bits("00000000")]                    # whole bytes: no padding
    stream = np.concatenate([p for p, _ in parts])
    got = V.finish_restart_scan(stream, [n for _, n in parts])
    want = (bytes([0b10110111]) + b"\xFF\xD0" + bytes([0xFF, 0x00, 0b01011111]) + b"\xFF\xD1" + bytes([0x01, 0xFF, 0x00]) + b"\xFF\xD2"
            + bytes([0xFF, 0x00]) + b"\xFF\xD3" + bytes([0x00]) + b"\xFF\xD9")
    assert got == want
    # the reference walk takes it apart again
    assert V.finish_restart_scan(stream[:1], [5]) == bytes([0b10110111]) + b"\xFF\xD9"      # one interval: no marker
    # the marker number wraps behind D7, and there is none behind the last interval
    eleven = V.finish_restart_scan(np.arange(1, 12, dtype=np.uint8), [8] * 11)
    assert eleven == b"".join(bytes([k + 1]) + (bytes([0xFF, 0xD0 + k % 8]) if k < 10 else b"") for k in range(11)) + b"\xFF\xD9"
    assert [eleven[i + 1] - 0xD0 for i in range(len(eleven) - 1) if eleven[i] == 0xFF and eleven[i + 1] != 0xD9] == [0, 1, 2, 3, 4, 5, 6, 7, 0, 1]
    # bytes behind the last interval are not the scan's
    assert V.finish_restart_scan(np.array([0x12, 0x34, 0x56], np.uint8), [8, 8]) == b"\x12\xFF\xD0\x34\xFF\xD9"
    # one interval is what finish_scan makes of it
    for p, n in parts:
        assert V.finish_restart_scan(p, [n]) == V.finish_scan(p, n)
    with pytest.raises(ValueError, match="at least one bit"):
        V.finish_restart_scan(stream, [5, 0, 3])


def test_written_scans_parse_back():
    """header + finish_restart_scan of the reference's interval streams is a file the reference walk, parse_jpeg and Pillow all read"""
    H, W, quality = 70, 38, 100
    t = V.jpeg_tables(quality)
    frames = R.make_frames("noise", 1, H, W)
    coefs, _ = R.blocks(frames, t.quant)
    plain = None
    for ri in (1, 4, 3, 15, 20):
        _, streams = RR.entropy_intervals(coefs, t.huff, ri)
        parts = [s[:(b + 7) // 8] for s, b in streams[0]]
        data = V.jpeg_header(H, W, quality, ri) + V.finish_restart_scan(np.concatenate(parts), [b for _, b in streams[0]])
        h, w, _, specs, got_ri, got_parts, markers = RR.split_restart_file(data)
        assert (h, w, got_ri) == (H, W, ri) and markers == [k % 8 for k in range(len(parts) - 1)] and len(got_parts) == len(parts)
        for (s, b), g in zip(streams[0], got_parts):                             # the same bytes up to the 1-bits that fill the last
            assert len(g) == (b + 7) // 8 and np.array_equal(np.unpackbits(g)[:b], np.unpackbits(s)[:b]) and np.unpackbits(g)[b:].all()
        assert np.array_equal(RR.decode_intervals(got_parts, specs, 15, ri), coefs[0])
        p = V.parse_jpeg(data, restart=True)
        assert p.restart == ri and all(np.array_equal(p.scan[p.intervals[k]:p.intervals[k + 1]], g) for k, g in enumerate(got_parts))
        pixels = R.decode(data)                                                  # Pillow opens it
        plain = pixels if plain is None else plain
        assert np.array_equal(pixels, plain) and np.array_equal(RR.decode(data), pixels)
    c0, s0, _ = R.entropy(coefs, t.huff)
    no_ri = V.jpeg_header(H, W, quality) + V.finish_scan(*s0[0])
    assert np.array_equal(R.decode(no_ri), plain)


def test_header_carries_the_interval():
    plain, ri = V.jpeg_header(24, 40, 90), V.jpeg_header(24, 40, 90, 300)
    assert V.jpeg_header(24, 40, 90, 0) == plain and b"\xFF\xDD" not in plain
    sos = plain.index(b"\xFF\xDA")
    assert ri == plain[:sos] + b"\xFF\xDD\x00\x04" + struct.pack(">H", 300) + plain[sos:]
    assert V.jpeg_header(24, 40, 90, 7) != ri and V.jpeg_header(24, 40, 90, 300) == ri      # the cache tells intervals apart
    with pytest.raises(ValueError, match="restart interval"):
        V.jpeg_header(24, 40, 90, 65536)


def test_restart_interval_validation():
    assert V.restart_mcus(None, 40) is None
    assert V.restart_mcus(1, 40) == 1 and V.restart_mcus(65535, 40) == 65535 and V.restart_mcus(np.int64(7), 40) == 7
    assert [V.restart_mcus("row", w) for w in (1, 16, 17, 38, 40, 512)] == [1, 1, 2, 3, 3, 32]
    for bad in (0, -1, 65536, 4.0, True, "rows", "4", (4,)):
        with pytest.raises(ValueError, match="restart_interval= takes None"):
            V.restart_mcus(bad, 40)
    # the writers check it before they touch a device or a file
    import torch
    frames = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    for bad in (0, -1, 65536, 4.0):
        with pytest.raises(ValueError, match="restart_interval= takes None"):
            V.encode_mjpeg(frames, 90, restart_interval=bad)


def test_call_save_restart_interval_refusals(tmp_path):
    from types import SimpleNamespace
    import torch
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    p = EMOAnimationPipeline(unet=SimpleNamespace(device=torch.device("cpu")), scheduler=DDIMScheduler())      # no VAE
    good = str(tmp_path / "clip.avi")
    for bad in (0, 65536, 4.0, "column"):
        with pytest.raises(ValueError, match="restart_interval= takes None"):
            p("", 2, save_path=good, fps=25, save_restart_interval=bad)
    for fine in (None, "row", 4):
        with pytest.raises(ValueError, match="VAE"):                             # the next check in line
            p("", 2, save_path=good, fps=25, save_restart_interval=fine)
    assert list(tmp_path.iterdir()) == []
