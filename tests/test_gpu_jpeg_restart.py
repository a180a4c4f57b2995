"""GPU tests of JPEG restart intervals (T.81 B.2.4.4, E.1.4): emo_jpeg_decode_segments (csrc/video_in.hip) and emo_jpeg_count_bits_ri /
emo_jpeg_emit_bits_ri (csrc/video_out.hip) against tests/jpeg_restart_ref.py (which tests/test_jpeg_restart_host.py holds to Pillow byte
for byte), then decode_mjpeg, encode_mjpeg(restart_interval=), write_video / read_video and the pipeline's save_restart_interval=
against Pillow itself.

Everything is integer arithmetic, so every comparison is an equality.  Every output a kernel writes is the front of a larger buffer whose
tail holds a poison value that must come back untouched; the coefficient fronts start out poisoned too, so a block a segment should
have written and did not shows."""
import numpy as np
import pytest
import torch

from emote_hack_amd import video_io as V
from tests import jpeg_decode_ref as D
from tests import jpeg_restart_ref as RR
from tests import mjpeg_ref as R
from tests.test_gpu_jpeg_decode import device_decode_tables, intact, poisoned
from tests.test_gpu_kernels import DEV, ops
from tests.test_gpu_mjpeg import POISON as BYTE_POISON, device_tables, env      # noqa: F401  (env: the tiny pipeline, a fixture)

pytestmark = pytest.mark.gpu
STAGE_BYTES = 4096                                       # JD_STAGE_BYTES: the window of a segment's stream a wave holds in LDS


def decode_segments(o, scan, seg_offsets, first, blocks, specs, n, n_mcu):
    """ops.jpeg_decode_segments into poisoned buffers -> (coefficients, status per segment) on the host"""
    n_seg = len(seg_offsets) - 1
    cb, coefs = poisoned((n, n_mcu, 6, 64), torch.int16)
    sb, status = poisoned((n_seg,), torch.int32)
    scan = np.concatenate([scan, np.zeros(-len(scan) % 4 or (0 if len(scan) else 4), np.uint8)])
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(DEV)
    o.jpeg_decode_segments(dev(scan, np.uint8), dev(seg_offsets, np.int64), dev(first, np.int32), dev(blocks, np.int32), device_decode_tables(specs),
                           n, n_mcu, out=coefs, status=status)
    torch.cuda.synchronize()
    assert intact((cb, coefs), (sb, status))
    return coefs.cpu().numpy(), status.cpu().numpy()


def interval_parts(coefs, huff, ri):
    """coefficients (n, MCUs, 6, 64) -> per frame the unstuffed bytes of every restart interval (the reference encoder's)"""
    return [[s[:(b + 7) // 8] for s, b in frame] for frame in RR.entropy_intervals(coefs, huff, ri)[1]]


# ------------------------------------------------------------------------------------------------------------------- the decoder kernel
@pytest.mark.parametrize("content", R.CONTENTS)
def test_decode_segments_equals_the_reference(content):
    o = ops()
    for n, H, W in R.SHAPES:
        frames = R.make_frames(content, n, H, W)
        n_mcu = int(np.prod(R.n_mcus(H, W)))
        for quality in RR.QUALITIES:
            t = V.jpeg_tables(quality)
            want, _ = R.blocks(frames, t.quant)
            for case in RR.RI_CASES:
                ri = RR.resolve(case, H, W)
                parts = interval_parts(want, t.huff, ri)
                assert [len(p) for p in parts] == [RR.n_intervals(n_mcu, ri)] * n
                got, status = decode_segments(o, *RR.segment_tables(parts, n_mcu, [ri] * n)[:4], t.specs, n, n_mcu)
                assert not status.any(), (content, n, H, W, quality, case, status)
                assert np.array_equal(got, want), (content, n, H, W, quality, case)
    assert RR.n_intervals(15, 1) > 9                     # Ri = 1 on the 15-MCU shape: the marker number of its file wraps


def test_a_segment_longer_than_the_window_beside_short_ones():
    """64 x 64 noise at quality 100: as one interval its 16 MCUs code about 8 KB, two windows; beside it in one launch the same frame cut
    into 16 intervals of one MCU, so the workgroup that holds the long segment holds segments of one MCU too, and frames without
    markers and with other intervals"""
    o = ops()
    frame = R.make_frames("noise", 1, 64, 64)
    t = V.jpeg_tables(100)
    want, _ = R.blocks(frame, t.quant)
    n_mcu = 16
    ris = [1, 16, 1, 0, 4, 5, 21]                        # 0: a frame without restart markers; 5 leaves a last interval of one MCU
    parts = [interval_parts(want, t.huff, ri or n_mcu)[0] for ri in ris]
    long_bytes = len(parts[1][0])
    assert len(parts[1]) == 1 and long_bytes > STAGE_BYTES, long_bytes
    scan, offsets, first, blocks, frame_of = RR.segment_tables(parts, n_mcu, ris)
    long_seg = int(np.flatnonzero(frame_of == 1)[0])
    group = np.arange(len(frame_of)) // 4 == long_seg // 4                      # the four segments of its workgroup
    assert sorted(set(blocks[group])) == [6, 96]
    got, status = decode_segments(o, scan, offsets, first, blocks, t.specs, len(ris), n_mcu)
    assert not status.any() and np.array_equal(got, np.repeat(want, len(ris), axis=0))
    # the segments in any order: where a segment's blocks go is the table's business alone
    order = np.random.default_rng(0).permutation(len(first))
    sizes = np.diff(offsets)
    scan2 = np.concatenate([scan[offsets[s]:offsets[s + 1]] for s in order])
    got, status = decode_segments(o, scan2, np.concatenate([[0], np.cumsum(sizes[order])]), first[order], blocks[order], t.specs, len(ris), n_mcu)
    assert not status.any() and np.array_equal(got, np.repeat(want, len(ris), axis=0))
    # two frames without markers of about 15 KB each: one wavefront walks a frame through several windows, and the product's path for
    # such frames (one workgroup per frame) gives the same
    frames = R.make_frames("noise", 2, 96, 128)
    want, _ = R.blocks(frames, t.quant)
    parts = interval_parts(want, t.huff, 48)
    assert min(len(p[0]) for p in parts) > 3 * STAGE_BYTES
    got, status = decode_segments(o, *RR.segment_tables(parts, 48, [0, 0])[:4], t.specs, 2, 48)
    assert not status.any() and np.array_equal(got, want)


def test_damaged_segments_report_and_return():
    o = ops()
    H, W, ri = 70, 38, 4
    t = V.jpeg_tables(90)
    n_mcu = 15
    want, _ = R.blocks(R.make_frames("ramp", 2, H, W), t.quant)
    parts = interval_parts(want, t.huff, ri)                                    # two frames of four intervals: 4, 4, 4 and 3 MCUs
    spans = RR.interval_mcus(n_mcu, ri)
    poison = np.int16(0x5A5A)

    def run(frame0_parts, n=2, mcus=n_mcu, table=None):
        scan, offsets, first, blocks, _ = RR.segment_tables([frame0_parts, parts[1]][:n], n_mcu, [ri] * n)
        if table is not None:
            offsets, first, blocks = table(offsets.copy(), first.copy(), blocks.copy())
        return decode_segments(o, scan, offsets, first, blocks, t.specs, n, mcus)

    def others_are_right(got, status, bad):
        for f in range(2):
            for k, (m0, m1) in enumerate(spans):
                if (f, k) != (0, bad):
                    assert status[f * 4 + k] == D.OK and np.array_equal(got[f, m0:m1], want[f, m0:m1]), (f, k)

    m0, m1 = spans[1]
    # interval 1 of frame 0 cut in half
    cut = parts[0][1][:len(parts[0][1]) // 2]
    got, status = run([parts[0][0], cut, parts[0][2], parts[0][3]])
    assert status[1] == D.PAST_END
    others_are_right(got, status, 1)
    seg = got[0, m0:m1].reshape(-1, 64)
    done = int(seg.any(axis=1).nonzero()[0].max()) + 1                          # the blocks in front of the cut are there, zeros behind
    assert 0 < done < len(seg) and np.array_equal(seg[:done - 1], want[0, m0:m1].reshape(-1, 64)[:done - 1]) and not seg[done:].any()
    # sixteen 1-bits in front of it are no code of any table
    got, status = run([parts[0][0], np.concatenate([np.array([0xFF, 0xFF], np.uint8), parts[0][1]]), parts[0][2], parts[0][3]])
    assert status[1] == D.BAD_CODE and not got[0, m0:m1].any()
    others_are_right(got, status, 1)
    # an empty segment
    got, status = run([parts[0][0], np.zeros(0, np.uint8), parts[0][2], parts[0][3]])
    assert status[1] == D.PAST_END and not got[0, m0:m1].any()
    others_are_right(got, status, 1)
    # a byte offset that leaves the scan: segment 0 ends with the buffer (what lies behind its blocks is not looked at), segment 1
    # starts there and runs backwards, an empty segment as well
    def wild_offsets(offsets, first, blocks):
        offsets[1] = 10 ** 12
        return offsets, first, blocks
    got, status = run(parts[0], table=wild_offsets)
    assert status[1] == D.PAST_END and not got[0, m0:m1].any()
    others_are_right(got, status, 1)
    # blocks that reach past the coefficient buffer: nothing is written behind it (decode_segments checks the poison), what fits decodes
    def reaching(offsets, first, blocks):
        blocks[3] += 600                                 # the frame's last interval claims 100 MCUs more
        return offsets, first, blocks
    got, status = run(parts[0], n=1, table=reaching)
    assert not status.any() and np.array_equal(got[0], want[0])
    got, status = run(parts[0], n=1, mcus=14)            # a buffer one MCU short: the last interval keeps two of its three MCUs
    assert not status.any() and np.array_equal(got[0], want[0, :14])
    def outside(offsets, first, blocks):
        first[2], blocks[1] = 10 ** 6, -12               # a segment that starts behind the buffer, one with a negative count: no blocks
        return offsets, first, blocks
    got, status = run(parts[0], n=1, table=outside)
    assert not status.any() and np.array_equal(got[0, :4], want[0, :4]) and np.array_equal(got[0, 12:], want[0, 12:])
    assert (got[0, 4:12] == poison).all()                # and what no segment names is not written


def test_entry_point_refusals():
    from emote_hack_amd._lib import EmoHipError
    o = ops()
    tables = device_decode_tables(V.HUFFMAN_SPECS)
    offsets = torch.zeros(2, device=DEV, dtype=torch.int64)
    one = torch.zeros(1, device=DEV, dtype=torch.int32)
    with pytest.raises(EmoHipError, match="multiple of 4"):
        o.jpeg_decode_segments(torch.zeros(30, device=DEV, dtype=torch.uint8), offsets, one, one, tables, 1, 1)
    with pytest.raises(EmoHipError, match="multiple of 4"):
        o.jpeg_decode_segments(torch.zeros(33, device=DEV, dtype=torch.uint8)[1:], offsets, one, one, tables, 1, 1)
    t, quant, huff = device_tables(90)
    coefs = torch.zeros(1, 1, 6, 64, device=DEV, dtype=torch.int16)
    lib = o._lib.load()
    counts = torch.zeros(6, device=DEV, dtype=torch.int32)
    for bad in (0, -3):
        assert lib.emo_jpeg_count_bits_ri(o._ptr(coefs), o._ptr(counts), 1, 1, bad, o._ptr(huff), o._stream()) != 0
        assert b"restart_mcus" in lib.emo_last_error_string()


# ------------------------------------------------------------------------------------------------------------------- the encoder kernels
def emit_intervals(o, coefs, huff, counts, ri):
    """what encode_streams does with an interval, on the host in numpy, into a buffer whose every byte behind the last stream byte holds
    BYTE_POISON -> (buffer, byte start (n, k), bits (n, k), total bytes)"""
    n, n_mcu = coefs.shape[:2]
    c = counts.cpu().numpy().astype(np.int64)
    spans = RR.interval_mcus(n_mcu, ri)
    bits = np.array([[c[f, m0 * 6:m1 * 6].sum() for m0, m1 in spans] for f in range(n)])
    nbytes = (bits + 7) // 8
    starts = (np.cumsum(nbytes.reshape(-1)) - nbytes.reshape(-1)).reshape(nbytes.shape)
    offsets = np.zeros_like(c)
    for f in range(n):
        for k, (m0, m1) in enumerate(spans):
            inside = c[f, m0 * 6:m1 * 6]
            offsets[f, m0 * 6:m1 * 6] = starts[f, k] * 8 + np.cumsum(inside) - inside
    total = int(nbytes.sum())
    words = (total + 3) // 4 * 4
    buf = torch.full((words + 64,), BYTE_POISON, device=DEV, dtype=torch.uint8)
    buf[:total] = 0
    o.jpeg_emit_bits(coefs, huff, torch.from_numpy(offsets).to(DEV), buf[:words], restart_mcus=ri)
    return buf.cpu().numpy(), starts, bits, total


@pytest.mark.parametrize("content", R.CONTENTS)
def test_encoder_kernels_with_an_interval(content):
    o = ops()
    for n, H, W in R.SHAPES:
        dev_frames = torch.from_numpy(R.make_frames(content, n, H, W)).to(DEV)
        n_mcu = int(np.prod(R.n_mcus(H, W)))
        for quality in RR.QUALITIES:
            t, quant, huff = device_tables(quality)
            coefs = o.jpeg_blocks(dev_frames, quant)
            host = coefs.cpu().numpy()
            plain = o.jpeg_count_bits(coefs, huff)
            assert np.array_equal(plain.cpu().numpy(), R.entropy(host, t.huff)[0])                  # the entry without an interval, as it was
            for case in RR.RI_CASES:
                what = f"{content} {n}x{H}x{W} q{quality} Ri {case}"
                ri = RR.resolve(case, H, W)
                ref_counts, ref_streams = RR.entropy_intervals(host, t.huff, ri)
                counts = o.jpeg_count_bits(coefs, huff, restart_mcus=ri)
                assert np.array_equal(counts.cpu().numpy(), ref_counts), what
                if ri >= n_mcu:
                    assert torch.equal(counts, plain), what
                buf, starts, bits, total = emit_intervals(o, coefs, huff, counts, ri)
                for f in range(n):
                    for k, (stream, nbits) in enumerate(ref_streams[f]):
                        assert int(bits[f, k]) == nbits and np.array_equal(buf[starts[f, k]:starts[f, k] + len(stream)], stream), (what, f, k)
                assert bool((buf[total:] == BYTE_POISON).all()), what
                # the product's path: the same bytes, framed
                dstream, dstarts, dbits = V.encode_streams(dev_frames, quality, restart_interval=ri)
                assert np.array_equal(dstarts, starts) and np.array_equal(dbits, bits) and np.array_equal(dstream.cpu().numpy()[:total], buf[:total]), what
                jpegs = V.encode_mjpeg(dev_frames, quality, restart_interval=ri)
                for f in range(n):
                    laid = np.concatenate([s[:(b + 7) // 8] for s, b in ref_streams[f]])
                    assert jpegs[f] == V.jpeg_header(H, W, quality, ri) + V.finish_restart_scan(laid, [b for _, b in ref_streams[f]]), (what, f)
            assert V.encode_mjpeg(dev_frames, quality, restart_interval=None) == V.encode_mjpeg(dev_frames, quality)


# ------------------------------------------------------------------------------------------------------------------- against Pillow
def test_decode_mjpeg_of_pillow_restart_files_equals_pillow():
    for H, W in [(16, 16), (24, 40), (70, 38), (64, 64)]:
        frame = R.make_frames("noise", 1, H, W)[0] if (H, W) == (64, 64) else D.picture(H, W, H * W)
        n_mcu = int(np.prod(R.n_mcus(H, W)))
        files = [RR.pillow_restart_file(frame, q, **kw) for q in RR.QUALITIES
                 for kw in (dict(blocks=1), dict(blocks=4), dict(blocks=n_mcu), dict(blocks=n_mcu + 5), dict(rows=1))]
        for f in files:
            got = V.decode_mjpeg([f])
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (1, H, W, 3)
            assert np.array_equal(got.cpu().numpy()[0], R.decode(f)), (H, W)
        # one call: three table sets, files with and without markers and with different intervals side by side
        mixed = files + [D.pillow_file(frame, 90, False), RR.pillow_restart_file(frame, 90, blocks=2, optimize=True), D.pillow_file(frame, 90, True)]
        assert np.array_equal(V.decode_mjpeg(mixed).cpu().numpy(), np.stack([R.decode(f) for f in mixed])), (H, W)


def test_encode_mjpeg_with_an_interval_round_trips():
    n, H, W = 3, 70, 38
    for content in ("ramp", "noise"):
        frames = torch.from_numpy(R.make_frames(content, n, H, W)).to(DEV)
        for quality in RR.QUALITIES:
            plain = np.stack([R.decode(j) for j in V.encode_mjpeg(frames, quality)])
            for case in RR.RI_CASES:
                ri = RR.resolve(case, H, W)
                jpegs = V.encode_mjpeg(frames, quality, restart_interval="row" if case == "row" else ri)
                for j in jpegs:
                    got_ri, parts, markers = RR.split_restart_file(j)[4:]
                    assert got_ri == ri and len(parts) == RR.n_intervals(15, ri) and markers == [k % 8 for k in range(len(parts) - 1)]
                pixels = np.stack([R.decode(j) for j in jpegs])                  # Pillow opens every file
                assert np.array_equal(pixels, plain), (content, quality, case)   # the same coefficients: the same pixels
                assert np.array_equal(V.decode_mjpeg(jpegs).cpu().numpy(), pixels), (content, quality, case)


def test_write_video_with_rows_reads_back(tmp_path):
    n, H, W = 5, 40, 56
    frames = torch.from_numpy(np.stack([D.picture(H, W, i) for i in range(n)])).to(DEV)
    path, plain_path = tmp_path / "rows.avi", tmp_path / "plain.avi"
    V.write_video(frames, str(path), 25, 90, restart_interval="row")
    V.write_video(frames, str(plain_path), 25, 90)
    jpegs, fps, _ = V.read_avi(path)
    assert len(jpegs) == n and fps == 25
    for j in jpegs:
        ri, parts = RR.split_restart_file(j)[4:6]
        assert ri == 4 and len(parts) == 3                                       # 56 pixels: 4 MCUs a row, 3 rows
    got, _, _ = V.read_video(path)
    assert np.array_equal(got.cpu().numpy(), np.stack([R.decode(j) for j in jpegs]))
    assert torch.equal(got, V.read_video(plain_path)[0])
    assert np.array_equal(np.stack(V.video2images(path, step=2, length=2, start=1)), got[1:5:2].cpu().numpy())
    V.images2video(frames.cpu().numpy(), str(tmp_path / "images.avi"), fps=25, restart_interval="row")
    assert V.read_avi(tmp_path / "images.avi")[0] == jpegs


def test_call_save_restart_interval_writes_dri(env, tmp_path):
    pipe, kw = env["pipe"], env["kw"]
    path = tmp_path / "clip.avi"
    got = pipe("", output_type="uint8", fps=25, save_path=str(path), save_restart_interval="row", **kw).videos
    jpegs, _, _ = V.read_avi(path)
    assert len(jpegs) == got.shape[1] == 4
    for j in jpegs:
        ri, parts = RR.split_restart_file(j)[4:6]
        assert ri == 8 and len(parts) == 8                                       # 128 x 128: 8 MCUs a row, 8 rows
    assert jpegs == V.encode_mjpeg(got, 90, restart_interval=8)
    assert torch.equal(V.read_video(path)[0], V.decode_mjpeg(V.encode_mjpeg(got, 90)))


def test_decode_mjpeg_names_the_frame_and_the_interval():
    n, H, W = 3, 70, 38
    frames = torch.from_numpy(R.make_frames("ramp", n, H, W)).to(DEV)
    jpegs = V.encode_mjpeg(frames, 90, restart_interval=4)
    data = jpegs[1]
    rst = [i for i in range(data.index(b"\xFF\xDA"), len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    assert len(rst) == 3
    mid = (rst[1] + 2 + rst[2]) // 2
    while data[mid - 1] == 0xFF:                                                 # not between an FF and its stuffed 00
        mid -= 1
    half = data[:rst[1] + 2] + data[rst[1] + 2:mid] + data[rst[2]:]              # interval 2 loses its second half
    with pytest.raises(ValueError, match=r"frame 1 does not decode: the scan ends .* in restart interval 2 of 4 \(emo_jpeg_decode_segments status 2\)"):
        V.decode_mjpeg([jpegs[0], half, jpegs[2]])
    ones = data[:rst[0] + 2] + b"\xFF\x00\xFF\x00" + data[rst[0] + 2:]                           # sixteen 1-bits in front of interval 1
    with pytest.raises(ValueError, match="frame 2 does not decode: a code the Huffman table does not define in restart interval 1 of 4"):
        V.decode_mjpeg([jpegs[0], jpegs[2], ones])
    with pytest.raises(ValueError, match="frame 0: parse_jpeg: 3 restart intervals in the scan"):
        V.decode_mjpeg([data[:rst[2]] + b"\xFF\xD9", jpegs[2]])
    plain = V.encode_mjpeg(frames, 90)                                           # a frame without markers names no interval
    with pytest.raises(ValueError, match=r"frame 1 does not decode: the scan ends before the frame's last block \(emo_jpeg_decode_segments"):
        V.decode_mjpeg([jpegs[0], plain[1][:(len(V.jpeg_header(H, W, 90)) + len(plain[1])) // 2] + b"\xFF\xD9"])
    assert np.array_equal(V.decode_mjpeg(jpegs).cpu().numpy(), np.stack([R.decode(j) for j in jpegs]))      # and the card is well
