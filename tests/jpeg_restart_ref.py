"""Test infrastructure, not product: restart intervals (T.81 B.2.4.4, E.1.4) on top of the numpy restatements tests/jpeg_decode_ref.py and
tests/mjpeg_ref.py.  A file is split at its RSTm markers by a byte-at-a-time walk of its own (nothing of emote_hack_amd.video_io is used);
an interval decodes as jpeg_decode_ref.huffman_decode(interval bytes, tables, MCUs of the interval) and encodes as
mjpeg_ref.entropy(coefficients of the interval's MCUs, tables): both exact, because the DC predictions start at 0 with every interval as
they do with a frame.  tests/test_jpeg_restart_host.py holds this to Pillow byte for byte; the GPU tests hold the kernels to it."""
import io

import numpy as np

from tests import jpeg_decode_ref as D
from tests import mjpeg_ref as R

RI_CASES = [1, 4, "row", "n_mcu", "n_mcu+5"]            # 4 divides neither the 6 MCUs of 24 x 40 nor the 15 of 70 x 38: a short last interval
QUALITIES = [10, 90, 100]


def resolve(ri, H, W):
    """a case of RI_CASES -> the restart interval in MCUs"""
    mr, mc = R.n_mcus(H, W)
    return {"row": mc, "n_mcu": mr * mc, "n_mcu+5": mr * mc + 5}.get(ri, ri)


def n_intervals(n_mcu, ri):
    return -(-n_mcu // min(ri, n_mcu))


def interval_mcus(n_mcu, ri):
    """[(first MCU, MCU behind the last)] of the restart intervals of a frame"""
    ri = min(ri, n_mcu)
    return [(m0, min(m0 + ri, n_mcu)) for m0 in range(0, n_mcu, ri)]


def pillow_restart_file(frame, quality, blocks=0, rows=0, optimize=False):
    """Pillow's baseline 4:2:0 file of one frame with a restart interval of `blocks` MCUs or `rows` MCU rows"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG", quality=quality, subsampling=2, optimize=optimize, restart_marker_blocks=blocks,
                                restart_marker_rows=rows)
    return buf.getvalue()


def split_restart_file(data):
    """a baseline 4:2:0 file -> (H, W, quant (2, 64) natural, four (BITS, HUFFVAL), Ri of its last DRI (0: none), [the unstuffed bytes of
    every restart interval], [m of every RSTm met]); the standard's byte-at-a-time rule (B.1.1.5), a walk of its own"""
    quant, huff = R.jpeg_tables_in(data)
    pos, ri = 2, 0
    while True:
        marker, size = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        if marker == 0xC0:
            H, W = int.from_bytes(data[pos + 5:pos + 7], "big"), int.from_bytes(data[pos + 7:pos + 9], "big")
            assert data[pos + 9] == 3 and data[pos + 11] == 0x22
            tq = [data[pos + 12], data[pos + 15]]
        if marker == 0xDD:
            assert size == 4
            ri = int.from_bytes(data[pos + 4:pos + 6], "big")
        pos += 2 + size
        if marker == 0xDA:
            break
    raw, parts, markers, cur, i = data[pos:], [], [], bytearray(), 0
    while True:
        if raw[i] != 0xFF:
            cur.append(raw[i])
            i += 1
        elif raw[i + 1] == 0x00:
            cur.append(0xFF)
            i += 2
        elif 0xD0 <= raw[i + 1] <= 0xD7:
            parts.append(np.frombuffer(bytes(cur), np.uint8))
            markers.append(raw[i + 1] - 0xD0)
            cur, i = bytearray(), i + 2
        else:
            parts.append(np.frombuffer(bytes(cur), np.uint8))
            break
    specs = [huff[(0, 0)], huff[(1, 0)], huff[(0, 1)], huff[(1, 1)]]
    return H, W, np.stack([quant[tq[0]], quant[tq[1]]]), specs, ri, parts, markers


def decode_intervals(parts, specs, n_mcu, ri):
    """the unstuffed intervals of one frame -> int16 (n_mcu, 6, 64): every interval on its own, from DC predictions 0"""
    spans = interval_mcus(n_mcu, ri) if ri else [(0, n_mcu)]
    assert len(parts) == len(spans), (len(parts), len(spans))
    return np.concatenate([D.huffman_decode(part, specs, m1 - m0) for part, (m0, m1) in zip(parts, spans)])


def decode(data):
    """one file, with or without restart intervals -> (H, W, 3) uint8, the whole restatement"""
    H, W, quant, specs, ri, parts, _ = split_restart_file(data)
    mr, mc = R.n_mcus(H, W)
    coefs = decode_intervals(parts, specs, mr * mc, ri)[None]
    return D.h2v2_rgb(*D.idct(coefs, quant, H, W), H, W)[0]


def entropy_intervals(coefs, huff, ri):
    """coefficients (n, MCUs, 6, 64) -> (bit counts int32 (n, MCUs * 6), [per frame: [(the interval's unstuffed stream as uint8 with zero
    bits behind the last, its bits)]]): mjpeg_ref.entropy of every interval's MCUs as a frame of their own"""
    coefs = np.asarray(coefs)
    n, n_mcu = coefs.shape[:2]
    counts, streams = np.zeros((n, n_mcu * 6), np.int32), [[] for _ in range(n)]
    for m0, m1 in interval_mcus(n_mcu, ri):
        c, s, _ = R.entropy(coefs[:, m0:m1], huff)
        counts[:, m0 * 6:m1 * 6] = c
        for f in range(n):
            streams[f].append(s[f])
    return counts, streams


def segment_tables(frames_parts, n_mcu, ris):
    """per frame: (its unstuffed intervals, its Ri or 0) -> (scan uint8, seg_offsets int64 (S + 1), seg_first_block int32 (S), seg_blocks
    int32 (S), frame of every segment): the tables emo_jpeg_decode_segments takes, built here independently of decode_mjpeg"""
    scan, offsets, first, blocks, frame = [], [0], [], [], []
    for f, (parts, ri) in enumerate(zip(frames_parts, ris)):
        spans = interval_mcus(n_mcu, ri) if ri else [(0, n_mcu)]
        assert len(parts) == len(spans)
        for part, (m0, m1) in zip(parts, spans):
            scan.append(np.asarray(part, np.uint8))
            offsets.append(offsets[-1] + len(part))
            first.append((f * n_mcu + m0) * 6)
            blocks.append((m1 - m0) * 6)
            frame.append(f)
    return (np.concatenate(scan) if scan else np.zeros(0, np.uint8), np.array(offsets, np.int64), np.array(first, np.int32),
            np.array(blocks, np.int32), np.array(frame))
