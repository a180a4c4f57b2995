"""GPU tests of progressive JPEG decoding: emo_jpeg_progressive_scan (csrc/video_in_progressive.hip) through its ops wrapper against
the serial decoder of tests/jpeg_progressive_ref.py (which tests/test_jpeg_progressive_host.py holds to Pillow byte for byte), and
decode_mjpeg / read_image / read_video / the pipeline under progressive=True against Pillow's decoder itself, with the device's own
baseline decode of the same picture as a second yardstick.  Pillow's default script on four layouts, restart intervals that change
from scan to scan, scripts Pillow never writes, mixed clips, damaged scans.

Everything but the VAE is integer arithmetic, so every comparison is an equality.  Every buffer the kernel writes is the front of a
larger one whose tail holds a poison value that must come back untouched."""
import functools
import io

import numpy as np
import pytest
import torch

from emote_hack_amd import video_io as V
from tests import jpeg_decode_ref as D
from tests import jpeg_layout_ref as L
from tests import jpeg_progressive_ref as P
from tests.test_gpu_jpeg_decode import intact, poisoned
from tests.test_gpu_kernels import DEV, ops

pytestmark = pytest.mark.gpu
SCRIPT_SIZES = [(9, 17), (38, 70)]


@functools.lru_cache(maxsize=None)
def pillow_case(name, H, W, quality, restart=()):
    """(Pillow's progressive file, the reference's split of it, the reference's coefficients): made once, shared, never written to"""
    pic = P.flat_picture() if (H, W) == P.FLAT else D.picture(H, W, H * W + quality)
    data = P.pillow_progressive(pic, name, quality, **dict(restart))
    f = P.split_progressive(data)
    return data, f, P.decode_coefficients(f)


@functools.lru_cache(maxsize=None)
def written_case(name, H, W, script, restart=True):
    """(a file the writer makes under `script` from the coefficients of Pillow's baseline file, its split, its coefficients, the baseline file)"""
    base = L.pillow_file(D.picture(H, W, H * W + 7), name, 90, False)
    b = L.split_file(base)
    data = P.write_progressive(L.coefficients(b), b["quant"], H, W, L.LAYOUTS[name], P.scripts(L.LAYOUTS[name][0], restart)[script])
    f = P.split_progressive(data)
    return data, f, P.decode_coefficients(f), base


def to_dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


def run_scans(o, splits, scans=None):
    """ops.jpeg_progressive_scan, one launch per scan in file order, over the frames `splits` (P.split_progressive dicts that share size,
    layout and script; tables and restart intervals may differ), from a segment table built HERE from the reference's split, into
    poisoned buffers -> (coefficients (n, n_mcu, bpm, 64), [status per segment] per scan) on the host"""
    f0 = splits[0]
    H, W, layout = f0["H"], f0["W"], f0["layout"]
    n, (mr, mc) = len(splits), L.grid(H, W, layout)
    cb, coefs = poisoned((n, mr * mc, L.bpm(layout), 64), torch.int16)
    coefs.zero_()
    statuses = []
    for k, sc0 in enumerate(f0["scans"][:scans]):
        comps = sc0["comps"]
        units = P.units_of(H, W, layout, comps)
        tables, parts, seg = [], [], []
        for f, split in enumerate(splits):
            sc = split["scans"][k]
            assert (sc["comps"], sc["Ss"], sc["Se"], sc["Ah"], sc["Al"]) == (comps, sc0["Ss"], sc0["Se"], sc0["Ah"], sc0["Al"])
            tabs = [0, 0, 0]
            if not (sc["Ss"] == 0 and sc["Ah"]):
                for j, (td, ta) in enumerate(sc["tables"]):
                    tabs[j] = len(tables)
                    tables.append(V.huffman_decode_table(*sc["huff"][(0, td) if sc["Ss"] == 0 else (1, ta)]))
            ri = sc["ri"] or units
            for i, part in enumerate(sc["parts"]):
                seg.append((f, i * ri, min((i + 1) * ri, units) - i * ri, tabs))
                parts.append(part)
        tables = tables or [np.zeros(o.JPEG_DECODE_TABLE_INTS, np.int32)]
        sizes = np.array([len(p) for p in parts], np.int64)
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        scan = np.concatenate(parts + [np.zeros(-int(offsets[-1]) % 4 or (0 if offsets[-1] else 4), np.uint8)])
        sb, status = poisoned((len(seg),), torch.int32)
        scan_comp = -1 if len(comps) == layout[0] and layout[0] > 1 else comps[0]
        o.jpeg_progressive_scan(to_dev(scan, np.uint8), to_dev(offsets, np.int64), to_dev([s[0] for s in seg], np.int32),
                                to_dev([s[1] for s in seg], np.int32), to_dev([s[2] for s in seg], np.int32), to_dev([s[3] for s in seg], np.int32),
                                to_dev(np.stack(tables), np.int32), coefs, H, W, layout, sc0["Ss"], sc0["Se"], sc0["Ah"], sc0["Al"], scan_comp,
                                status=status)
        torch.cuda.synchronize()
        assert intact((cb, coefs), (sb, status))
        statuses.append(status.cpu().numpy())
    return coefs.cpu().numpy(), statuses


def device_baseline(pic, name, quality):
    """the second yardstick: the device's decode of the baseline file of the same picture, quality and layout"""
    return V.decode_mjpeg([L.pillow_file(pic, name, quality, False)]).cpu().numpy()[0]


# ------------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("name", list(L.LAYOUTS))
def test_scan_kernel_fills_the_coefficient_buffer_as_the_reference_decoder(name):
    o = ops()
    for H, W in P.SIZES:
        for quality in P.QUALITIES:
            data, f, want = pillow_case(name, H, W, quality)
            got, statuses = run_scans(o, [f])
            assert all(not s.any() for s in statuses), (H, W, quality, statuses)
            assert np.array_equal(got[0], want), (H, W, quality)


def test_scan_kernel_after_every_scan_of_the_progression():
    """the buffer after 1, 2, .. scans: every procedure is held to the reference on its own, not only the sum of them"""
    o = ops()
    data, f, _ = pillow_case("4:2:0", 9, 17, 100)
    for k in range(1, len(f["scans"]) + 1):
        got, _ = run_scans(o, [f], scans=k)
        assert np.array_equal(got[0], P.decode_coefficients(f, scans=k)), k


def test_scan_kernel_unit_mapping_leaves_padding_blocks_alone():
    """9 x 17 at 4:2:0: the luminance scans walk 3 x 2 blocks inside the 4 x 2 of the MCU grid; the blocks they never visit keep the DC
    of the interleaved scans and no AC coefficient"""
    o = ops()
    _, f, want = pillow_case("4:2:0", 9, 17, 90)
    got, _ = run_scans(o, [f])
    assert got.shape == (1, 2, 6, 64) and np.array_equal(got[0], want)
    assert not got[0, 1, 1, 1:].any() and not got[0, 1, 3, 1:].any() and got[0, 0, :4, 1:].any() and got[0, 1, 0, 1:].any()


def test_scan_kernel_reads_long_eob_runs():
    o = ops()
    _, f, want = pillow_case("4:4:4", *P.FLAT, 90)
    got, statuses = run_scans(o, [f])
    assert all(not s.any() for s in statuses) and np.array_equal(got[0], want)
    assert want.shape[0] == 272 and not want[:, :, 1:].any() and want[:, :, 0].all()


@pytest.mark.parametrize("name", list(L.LAYOUTS))
def test_scan_kernel_with_restart_intervals(name):
    o = ops()
    for H, W in SCRIPT_SIZES:
        for kw in (dict(restart_marker_rows=1), dict(restart_marker_blocks=1)):
            _, f, want = pillow_case(name, H, W, 90, tuple(kw.items()))
            assert any(len(sc["parts"]) > 1 for sc in f["scans"])
            got, statuses = run_scans(o, [f])
            assert all(not s.any() for s in statuses) and np.array_equal(got[0], want), (H, W, kw)
            assert np.array_equal(want, pillow_case(name, H, W, 90)[2])             # the same coefficients as without intervals
        # the writer's interval of 3 units, on some scans only; and the same file written without
        _, f, want, _ = written_case(name, H, W, "restart")
        _, plain, want_plain, _ = written_case(name, H, W, "restart", False)
        assert [sc["ri"] for sc in f["scans"]][:3] == [3, 0, 3] and np.array_equal(want, want_plain)
        for split in (f, plain):
            got, statuses = run_scans(o, [split])
            assert all(not s.any() for s in statuses) and np.array_equal(got[0], want), (H, W)


@pytest.mark.parametrize("name", list(L.LAYOUTS))
def test_scan_kernel_on_scripts_pillow_never_writes(name):
    o = ops()
    for H, W in SCRIPT_SIZES:
        for script in P.scripts(L.LAYOUTS[name][0]):
            data, f, want, base = written_case(name, H, W, script)
            got, statuses = run_scans(o, [f])
            assert all(not s.any() for s in statuses) and np.array_equal(got[0], want), (H, W, script)
            rgb = V.decode_mjpeg([data], progressive=True).cpu().numpy()[0]
            assert np.array_equal(rgb, L.pillow_decode(data)) and np.array_equal(rgb, L.pillow_decode(base)), (H, W, script)


def test_scan_kernel_takes_many_frames_with_their_own_tables():
    o = ops()
    splits = [pillow_case("4:2:2", 38, 70, q, r)[1] for q, r in ((90, ()), (10, ()), (100, (("restart_marker_rows", 1),)))]
    got, statuses = run_scans(o, splits)
    assert all(not s.any() for s in statuses)
    for i, (q, r) in enumerate(((90, ()), (10, ()), (100, (("restart_marker_rows", 1),)))):
        assert np.array_equal(got[i], pillow_case("4:2:2", 38, 70, q, r)[2]), i


def test_wrapper_checks_its_arguments_before_any_launch():
    o = ops()
    z = lambda *shape, dtype=torch.int32: torch.zeros(*shape, device=DEV, dtype=dtype)
    args = lambda **kw: {**dict(scan=z(4, dtype=torch.uint8), seg_offsets=z(2, dtype=torch.int64), seg_frame=z(1), seg_first_unit=z(1), seg_units=z(1),
                                seg_tables=z(1, 3), tables=z(1, o.JPEG_DECODE_TABLE_INTS), coefs=z(1, 2, 6, 64, dtype=torch.int16), H=9, W=17,
                                layout=(3, 2, 2), Ss=0, Se=0, Ah=0, Al=0, scan_comp=-1), **kw}
    o.jpeg_progressive_scan(**args())
    for bad in (dict(Se=5), dict(Ss=1, Se=5), dict(Ss=6, Se=5, scan_comp=0), dict(Ss=1, Se=64, scan_comp=0), dict(Al=14), dict(Ah=2, Al=0),
                dict(scan_comp=3), dict(layout=(3, 1, 2)), dict(coefs=z(1, 3, 6, 64, dtype=torch.int16)), dict(seg_tables=z(1, 4)),
                dict(tables=z(1, 64)), dict(seg_frame=z(2))):
        with pytest.raises(AssertionError):
            o.jpeg_progressive_scan(**args(**bad))


# ------------------------------------------------------------------------------------------------------------------- against Pillow
@pytest.mark.parametrize("name", list(L.LAYOUTS))
def test_decode_mjpeg_equals_pillow_and_the_baseline_decode(name):
    for H, W in P.SIZES:
        for quality in P.QUALITIES:
            data = pillow_case(name, H, W, quality)[0]
            got = V.decode_mjpeg([data], progressive=True)
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (1, H, W, 3)
            assert np.array_equal(got.cpu().numpy()[0], L.pillow_decode(data)), (H, W, quality)
            assert np.array_equal(got.cpu().numpy()[0], device_baseline(D.picture(H, W, H * W + quality), name, quality)), (H, W, quality)
    for H, W in SCRIPT_SIZES:
        for kw in (dict(restart_marker_rows=1), dict(restart_marker_blocks=1)):
            data = pillow_case(name, H, W, 90, tuple(kw.items()))[0]
            assert np.array_equal(V.decode_mjpeg([data], progressive=True).cpu().numpy()[0], L.pillow_decode(data)), (H, W, kw)


def mixed_clip():
    H, W = 38, 70
    pics = [D.picture(H, W, 20 + i) for i in range(7)]
    files = [L.pillow_file(pics[0], "4:2:0", 90, False), P.pillow_progressive(pics[1], "4:2:0", 90), P.pillow_progressive(pics[2], "4:2:2", 90),
             P.pillow_progressive(pics[3], "grey", 90), P.pillow_progressive(pics[4], "4:2:0", 90), P.pillow_progressive(pics[5], "4:2:2", 90, restart_marker_rows=1),
             L.pillow_file(pics[6], "grey", 90, True)]
    return files


def test_decode_mjpeg_mixes_baseline_and_progressive_frames():
    files = mixed_clip()
    parsed = [V.parse_jpeg(d, progressive=True) for d in files]
    assert [p.scans is not None for p in parsed] == [False, True, True, True, True, True, False]
    # frames 1 and 4, and 2 and 5, share a group: one script, their own optimised Huffman tables, one of them with restart intervals
    assert parsed[1].table_key() == parsed[4].table_key() and parsed[2].table_key() == parsed[5].table_key()
    assert parsed[1].scans[1].specs != parsed[4].scans[1].specs and parsed[5].scans[0].restart and not parsed[2].scans[0].restart
    assert len({p.table_key() for p in parsed}) == 5
    got = V.decode_mjpeg(files, progressive=True)
    assert tuple(got.shape) == (7, 38, 70, 3)
    assert np.array_equal(got.cpu().numpy(), np.stack([L.pillow_decode(d) for d in files]))
    with pytest.raises(ValueError, match="decode_mjpeg: frame 1: parse_jpeg: a progressive \\(SOF2\\) file"):
        V.decode_mjpeg(files)


def test_read_video_and_load_control_clip_take_progressive_frames(tmp_path):
    files = mixed_clip()                  # baseline 4:2:0 and grey, progressive 4:2:0, 4:2:2 and grey: five groups, one and three components
    path = str(tmp_path / "mixed.avi")
    V.write_avi(path, files, 70, 38, 25)
    frames, fps, _ = V.read_video(path, progressive=True)
    want = np.stack([L.pillow_decode(d) for d in files])
    assert frames.is_cuda and fps == 25 and tuple(frames.shape) == (7, 38, 70, 3) and np.array_equal(frames.cpu().numpy(), want)
    clip, length = V.load_control_clip(path, (70, 38), 4, progressive=True)
    assert length == 7 and tuple(clip.shape) == (8, 38, 70, 3) and np.array_equal(clip[:7].cpu().numpy(), want)
    assert np.array_equal(clip[7].cpu().numpy(), want[6])                        # padded with the last frame to whole windows
    with pytest.raises(ValueError, match="frame 1: parse_jpeg: a progressive"):
        V.read_video(path)


# ------------------------------------------------------------------------------------------------------------------- damaged scans
def _replace_scan(data, k, change):
    """the file with the entropy-coded bytes of scan k (no restart markers in it) replaced by change(those bytes, unstuffed), restuffed"""
    pos, seen = 2, -1
    while True:
        size = int.from_bytes(data[pos + 2:pos + 4], "big")
        if data[pos + 1] == 0xDA:
            seen += 1
            start = end = pos + 2 + size
            while not (data[end] == 0xFF and data[end + 1] != 0x00):
                end += 1
            if seen == k:
                raw = data[start:end].replace(b"\xFF\x00", b"\xFF")
                return data[:start] + bytes(change(raw)).replace(b"\xFF", b"\xFF\x00") + data[end:]
            pos = end
        else:
            pos += 2 + size


def _ac_scan_of(codes_and_bits, spec):
    """an AC scan's bytes from [(symbol, extra bits value, extra bit count)], coded with the table `spec`, padded with 1-bits"""
    code = P._codes(spec)
    out = P._Bits()
    for sym, extra, n in codes_and_bits:
        out.put(*code[sym])
        out.put(extra, n)
    b = out.bits + [1] * (-len(out.bits) % 8)
    return np.packbits(np.array(b, np.uint8)).tobytes()


def test_damaged_scans_come_back_as_errors_that_name_frame_and_scan():
    """damaged DATA for a kernel whose loops are all counted: each ends in a status, the other frames of the clip decode"""
    H, W = 38, 70
    good = [P.pillow_progressive(D.picture(H, W, 30 + i), "4:4:4", 90) for i in range(3)]
    want = [L.pillow_decode(d) for d in good]
    p = V.parse_jpeg(good[1], progressive=True)
    assert p.scans[4].script == ((0,), 6, 63, 0, 2) and p.scans[1].script == ((0,), 1, 5, 0, 2)
    all_ones = lambda raw: b"\xFF" * len(raw)                                     # no code is all 1-bits (Annex C)
    own = P.TABLES["acA"]                                                          # the hand-made scans are coded with the writer's table
    cases = [
        (lambda raw: raw[:len(raw) // 2], False, "the scan ends before the frame's last block", 2),
        (all_ones, False, "a code the Huffman table does not define", 1),
        # a run of 15 zeros and a coefficient, five times: the fourth leaves the band 6 .. 63 at position 69
        (lambda raw: _ac_scan_of([(0xF1, 1, 1)] * 5, own), True, "a zero run leaves its block", 3),
        # EOB14 with all extra bits set: a run of 32767 blocks in a scan of 45
        (lambda raw: _ac_scan_of([(0xE0, (1 << 14) - 1, 14)], own), True, "a zero run leaves its block", 3),
    ]
    k, s = 4, p.scans[4]
    for change, own_table, says, status in cases:
        bad = _replace_scan(good[1], k, change)
        if own_table:                                                            # a DHT right in front of the scan's SOS puts it at the scan's destination
            at = _scan_positions(bad)[k]
            bad = bad[:at] + P._seg(0xC4, bytes([0x10 | s.huffman[0][1]]) + bytes(own[0]) + own[1]) + bad[at:]
        with pytest.raises(ValueError, match=f"decode_mjpeg: frame 1 does not decode: {says} in scan {k} of 10 \\({s.Ss}\\.\\.{s.Se}, Ah/Al {s.Ah}/{s.Al}\\) "
                                             f"\\(emo_jpeg_progressive_scan status {status}\\)"):
            V.decode_mjpeg([good[0], bad, good[2]], progressive=True)
    # a frame cut into restart intervals: the error names the interval too (scan 1, luminance 1 .. 5: 45 blocks in 5 rows of 9)
    rows = P.pillow_progressive(D.picture(H, W, 31), "4:4:4", 90, restart_marker_rows=1)
    assert [len(x.intervals) - 1 for x in V.parse_jpeg(rows, progressive=True).scans][:2] == [5, 5]
    with pytest.raises(ValueError, match="decode_mjpeg: frame 2 does not decode: a code the Huffman table does not define in scan 1 of 10 "
                                         "\\(1\\.\\.5, Ah/Al 0/2\\) in restart interval 3 of 5 \\(emo_jpeg_progressive_scan status 1\\)"):
        V.decode_mjpeg([good[0], rows, _replace_interval(rows, 1, 3, b"\xFF\x00" * 4)], progressive=True)
    # the next call on the same device decodes the good frames: an error ends a segment, nothing else
    got = V.decode_mjpeg(good, progressive=True).cpu().numpy()
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def _replace_interval(data, k, i, new):
    """the file with restart interval i of scan k replaced by the (stuffed) bytes `new`"""
    at = _scan_positions(data)[k]
    begin = pos = at + 2 + int.from_bytes(data[at + 2:at + 4], "big")
    spans = []
    while True:
        if data[pos] == 0xFF and data[pos + 1] != 0x00:
            spans.append((begin, pos))
            if not 0xD0 <= data[pos + 1] <= 0xD7:
                break
            begin = pos = pos + 2
        else:
            pos += 1
    return data[:spans[i][0]] + new + data[spans[i][1]:]


def _scan_positions(data):
    pos, out = 2, []
    while data[pos + 1] != 0xD9:
        size = int.from_bytes(data[pos + 2:pos + 4], "big")
        if data[pos + 1] == 0xDA:
            out.append(pos)
            pos += 2 + size
            while not (data[pos] == 0xFF and data[pos + 1] != 0x00 and not 0xD0 <= data[pos + 1] <= 0xD7):
                pos += 1
        else:
            pos += 2 + size
    return out


DAMAGE = {   # what replaces the bytes of scan 4 (luminance 6 .. 63, first), whether it is coded with the writer's table acA, the status
    "a scan cut short": (lambda raw: raw[:len(raw) // 2], False, D.PAST_END),
    # no code is all 1-bits (Annex C); 4 bytes of them, because with fewer than 16 bits left in a segment a code that matches nothing counts
    # as cut short (the middle frame's scan at quality 10 is shorter than that)
    "an undefined code": (lambda raw: b"\xFF" * max(len(raw), 4), False, D.BAD_CODE),
    "a zero run that leaves the band": (lambda raw: _ac_scan_of([(0xF1, 1, 1)] * 5, P.TABLES["acA"]), True, D.BAD_RUN),
    "an EOB run longer than the segment": (lambda raw: _ac_scan_of([(0xE0, (1 << 14) - 1, 14)], P.TABLES["acA"]), True, D.BAD_RUN),
}


@pytest.mark.parametrize("kind", list(DAMAGE))
def test_a_damaged_segment_leaves_the_other_segments_of_the_launch_alone(kind):
    """kernel level: three frames in one launch per scan, the middle one's scan 4 damaged; its status says how, the other frames'
    status is 0 and their coefficients are the reference's, nothing is written outside the buffers (run_scans checks the poison)"""
    o = ops()
    change, own_table, status = DAMAGE[kind]
    splits = [dict(pillow_case("4:4:4", 38, 70, q)[1]) for q in (90, 10, 100)]
    cut = dict(splits[1]["scans"][4])
    assert (cut["comps"], cut["Ss"], cut["Se"], cut["Ah"]) == ((0,), 6, 63, 0)
    cut["parts"] = [np.frombuffer(bytes(change(cut["parts"][0].tobytes())), np.uint8)]
    if own_table:
        cut["huff"] = {**cut["huff"], (1, cut["tables"][0][1]): P.TABLES["acA"]}
    splits[1]["scans"] = splits[1]["scans"][:4] + [cut] + splits[1]["scans"][5:]
    got, statuses = run_scans(o, splits)
    assert list(statuses[4]) == [0, status, 0] and not any(s.any() for i, s in enumerate(statuses) if i < 4)
    assert all(s[0] == 0 and s[2] == 0 for s in statuses)                         # the later scans too, for the frames beside it
    assert np.array_equal(got[0], pillow_case("4:4:4", 38, 70, 90)[2]) and np.array_equal(got[2], pillow_case("4:4:4", 38, 70, 100)[2])


# ------------------------------------------------------------------------------------------------------------------- the surface
def test_read_image_takes_progressive_files(tmp_path):
    from PIL import Image
    for name in L.LAYOUTS:
        data = pillow_case(name, 38, 70, 90)[0]
        path = tmp_path / f"still_{name.replace(':', '')}.jpg"
        path.write_bytes(data)
        for src in (data, str(path)):
            got = V.read_image(src, progressive=True)
            assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), L.pillow_decode(data)), name
    data = pillow_case("4:2:0", 38, 70, 90)[0]
    for size, resample, pil in (((64, 64), "bicubic", Image.BICUBIC), ((40, 24), "bilinear", Image.BILINEAR)):
        want = np.array(Image.open(io.BytesIO(data)).convert("RGB").resize(size, pil))
        got = V.read_image(data, size=size, resample=resample, progressive=True)
        assert tuple(got.shape) == (size[1], size[0], 3) and np.array_equal(got.cpu().numpy(), want), size
    cut = data[:_scan_positions(data)[6]] + b"\xFF\xD9"
    with pytest.raises(ValueError, match="read_image: parse_jpeg: the progression is not complete"):
        V.read_image(cut, progressive=True)


@pytest.fixture(scope="module")
def pipe():
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    from tests import cases
    from tests.test_gpu_unet import build
    from tests.test_gpu_vae import SMALL, build as build_vae
    return EMOAnimationPipeline(vae=build_vae(SMALL, torch.float32)[0], unet=build(cases.TINY_MOTION, torch.float32), scheduler=DDIMScheduler())


def pillow_source_image(path, width, height):
    from PIL import Image
    return np.array(Image.open(path).convert("RGB").resize((width, height)))


def test_source_image_from_a_progressive_jpeg_stays_on_the_device(pipe, tmp_path):
    pic = D.picture(96, 120, 4)
    for name in L.LAYOUTS:
        path = str(tmp_path / f"portrait_{name.replace(':', '')}.jpg")
        open(path, "wb").write(P.pillow_progressive(pic, name, 90))
        for width, height in ((64, 64), (120, 96)):
            rgb = pipe._source_image_rgb(path, width, height, None, True)
            assert torch.is_tensor(rgb) and rgb.is_cuda and rgb.dtype == torch.uint8
            assert np.array_equal(rgb.cpu().numpy(), pillow_source_image(path, width, height)), (name, width, height)
        assert isinstance(pipe._source_image_rgb(path, 64, 64), np.ndarray)       # without the keyword: Pillow's, as before
    path = str(tmp_path / "portrait_420.jpg")
    from_path = pipe._source_image_latents(path, 64, 64, None, True)
    from_array = pipe._source_image_latents(pillow_source_image(path, 64, 64), 64, 64)
    assert from_path.is_cuda and tuple(from_path.shape) == (1, 4, 8, 8) and float(from_path.abs().max()) > 0
    # the bound of test_source_image_from_a_still_jpeg_stays_on_the_device: the pixels are equal, the two roads to the VAE differ in float32 order
    assert torch.allclose(from_path, from_array.to(from_path.device), rtol=1e-3, atol=1e-4), float((from_path - from_array.to(from_path.device)).abs().max())
    # what is still refused stays Pillow's: an incomplete progression, a PNG
    data = open(path, "rb").read()
    cut = str(tmp_path / "cut.jpg")
    open(cut, "wb").write(data[:_scan_positions(data)[6]] + b"\xFF\xD9")
    rgb = pipe._source_image_rgb(cut, 64, 64, None, True)
    assert isinstance(rgb, np.ndarray) and np.array_equal(rgb, pillow_source_image(cut, 64, 64))


def test_pipeline_call_with_input_progressive(pipe, tmp_path):
    """__call__(input_progressive=True, source_image=<progressive file>) == the same call fed the Pillow-decoded array.  The reference
    latents of the two calls differ as in the test above (equal pixels, two float32 roads into the VAE: rtol 1e-3 / atol 1e-4); two
    denoising steps carry that through the tiny UNet, for which tests/test_gpu_vae.py's source-image test allows rtol 2e-3 / atol 2e-4."""
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from tests import cases
    from tests.test_gpu_unet import build as build_unet
    from emote_hack_amd.synth import seeded_randn
    ref = build_unet(cases.TINY, torch.float32, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    path = str(tmp_path / "portrait.jpg")
    open(path, "wb").write(P.pillow_progressive(D.picture(96, 120, 4), "4:2:0", 90))
    kw = dict(height=64, width=64, num_inference_steps=2, appearance_encoder=ref, context_frames=4, init_latents=seeded_randn((4, 4, 8, 8), 5),
              text_embeddings=seeded_randn((2, 5, 32), 2), output_type="latent")
    a = pipe("", 4, source_image=path, input_progressive=True, **kw).videos
    b = pipe("", 4, source_image=pillow_source_image(path, 64, 64), **kw).videos
    assert tuple(a.shape) == (1, 4, 4, 8, 8) and bool(torch.isfinite(a).all())
    torch.testing.assert_close(a.cpu(), b.cpu(), rtol=2e-3, atol=2e-4)
    with pytest.raises(ValueError, match="input_progressive= takes True or False"):
        pipe("", 4, source_image=path, input_progressive="yes", **kw)
