"""What the PNG tests measure against, in numpy and plain Python, written from the header comment of include/emo_hip.h and independent of
the kernels: the five filters with the adaptive choice, the Adler-32 pair of every filtered row, the greedy single-probe LZ77 of every
strip with its histogram, and the bit stream of a frame's one dynamic block given its code tables (the tables themselves come from
emote_hack_amd.video_io.deflate_tables, which the host tests check on their own).  The containers are restated here too, so a file is
compared byte for byte."""
import struct
import zlib

import numpy as np

ADLER = 65521
# RFC 1951 3.2.5, written out: (first length, extra bits) of symbols 257 .. 285 and (first distance, extra bits) of symbols 0 .. 29
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def length_symbol(length):
    """3 .. 258 -> (symbol 257 .. 285, extra bits, their value)"""
    if length == 258:
        return 285, 0, 0
    k = max(i for i in range(28) if LENGTH_BASE[i] <= length)
    return 257 + k, LENGTH_EXTRA[k], length - LENGTH_BASE[k]


def distance_symbol(dist):
    """1 .. 32768 -> (symbol 0 .. 29, extra bits, their value)"""
    k = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return k, DIST_EXTRA[k], dist - DIST_BASE[k]


# ------------------------------------------------------------------------------------------------------------------------------ filter
def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def filter_row(t, raw, above, C):
    """raw, above: uint8 (W * C) (above: zeros for row 0) -> uint8 (W * C), the row filtered with type t"""
    x = raw.astype(np.int64)
    a = np.concatenate([np.zeros(C, np.int64), x[:-C]]) if len(x) > C else np.zeros(len(x), np.int64)
    b = above.astype(np.int64)
    c = np.concatenate([np.zeros(C, np.int64), b[:-C]]) if len(x) > C else np.zeros(len(x), np.int64)
    if t == 0:
        pred = np.zeros_like(x)
    elif t == 1:
        pred = a
    elif t == 2:
        pred = b
    elif t == 3:
        pred = (a + b) // 2
    else:
        pred = np.array([paeth(int(ai), int(bi), int(ci)) for ai, bi, ci in zip(a, b, c)], np.int64).reshape(x.shape)
    return ((x - pred) % 256).astype(np.uint8)


def filter_frames(frames, filter):
    """(n, H, W, C) uint8 -> uint8 (n, H, 1 + W * C): filter 0 .. 4 forced, 5 the smallest sum of min(v, 256 - v), the lowest type on a tie"""
    n, H, W, C = frames.shape
    out = np.zeros((n, H, 1 + W * C), np.uint8)
    for f in range(n):
        for y in range(H):
            raw = frames[f, y].reshape(-1)
            above = frames[f, y - 1].reshape(-1) if y else np.zeros(W * C, np.uint8)
            if filter == 5:
                rows = [filter_row(t, raw, above, C) for t in range(5)]
                costs = [int(np.minimum(r.astype(np.int64), 256 - r.astype(np.int64)).sum()) for r in rows]
                t = costs.index(min(costs))                                      # index keeps the first of equals
                row = rows[t]
            else:
                t, row = filter, filter_row(filter, raw, above, C)
            out[f, y, 0], out[f, y, 1:] = t, row
    return out


def adler_pairs(filtered):
    """uint8 (n, H, R) -> int64 (n, H, 2): per row s1 = (1 + sum d_i) mod 65521, s2 = (R + sum (R - i) d_i) mod 65521"""
    R = filtered.shape[-1]
    d = filtered.astype(object)
    weights = np.arange(R, 0, -1).astype(object)
    s1 = (1 + d.sum(axis=-1)) % ADLER
    s2 = (R + (d * weights).sum(axis=-1)) % ADLER
    return np.stack([s1, s2], axis=-1).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------------------ tokens
def hash3(s, pos):
    return (((s[pos] | s[pos + 1] << 8 | s[pos + 2] << 16) * 0x9E3779B1) & 0xFFFFFFFF) >> 20


def tokenize_strip(s):
    """bytes of one strip -> tokens: an int for a literal, (length, distance) for a match"""
    s, P = bytes(s), len(s)
    table, pos, out = {}, 0, []
    while pos < P:
        token = s[pos]
        if pos + 3 <= P:
            h = hash3(s, pos)
            cand = table.get(h)
            table[h] = pos
            if cand is not None and pos - cand <= 32768:
                limit, L = min(258, P - pos), 0
                while L < limit and s[cand + L] == s[pos + L]:
                    L += 1
                if L >= 3:
                    token = (L, pos - cand)
        out.append(token)
        pos += token[0] if isinstance(token, tuple) else 1
    return out


def strips_of(filtered_frame, strip_rows):
    """uint8 (H, R) -> the byte strings of its strips"""
    H = filtered_frame.shape[0]
    rows = H if strip_rows is None else min(int(strip_rows), H)
    return [filtered_frame[r0:r0 + rows].tobytes() for r0 in range(0, H, rows)]


def tokenize_frame(filtered_frame, strip_rows):
    """-> (tokens per strip, hist int64 (320): literal / length symbols at 0 .. 285 with one end-of-block at 256, distances at 288 + d)"""
    strips = [tokenize_strip(s) for s in strips_of(filtered_frame, strip_rows)]
    hist = np.zeros(320, np.int64)
    for tokens in strips:
        for t in tokens:
            if isinstance(t, tuple):
                hist[length_symbol(t[0])[0]] += 1
                hist[288 + distance_symbol(t[1])[0]] += 1
            else:
                hist[t] += 1
    hist[256] += 1
    return strips, hist


def packed(tokens):
    """tokens -> uint32 as the device packs them: length << 16 | distance, or the literal byte"""
    return np.array([t[0] << 16 | t[1] if isinstance(t, tuple) else t for t in tokens], np.uint32)


# ------------------------------------------------------------------------------------------------------------------------------ stream
class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n, self.bits = bytearray(), 0, 0, 0

    def put(self, value, width):
        self.acc |= value << self.n
        self.n += width
        self.bits += width
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def put_huffman(w, code, length):
    """a canonical code goes on the wire most significant bit first"""
    for k in range(length - 1, -1, -1):
        w.put((code >> k) & 1, 1)


def zlib_stream(filtered_frame, strip_rows, tables):
    """One frame's zlib stream: 78 01, ONE dynamic block - tables.header, the tokens of all strips end to end, the end-of-block - zero bits
    to the next byte, the Adler-32 big-endian.  tables: video_io.DeflateTables; only its lengths and its header are used: the codes
    are rebuilt here from the lengths as RFC 1951 3.2.2 says."""
    strips, _ = tokenize_frame(filtered_frame, strip_rows)
    lengths = [int(l) for l in tables.lengths]
    lit, dist = canonical(lengths[:286]), canonical(lengths[288:318])
    w = BitWriter()
    w.put(0x78, 8)
    w.put(0x01, 8)
    w.put(tables.header, tables.header_bits)
    for tokens in strips:
        for t in tokens:
            if isinstance(t, tuple):
                sym, nx, x = length_symbol(t[0])
                put_huffman(w, lit[sym], lengths[sym])
                w.put(x, nx)
                sym, nx, x = distance_symbol(t[1])
                put_huffman(w, dist[sym], lengths[288 + sym])
                w.put(x, nx)
            else:
                put_huffman(w, lit[t], lengths[t])
    put_huffman(w, lit[256], lengths[256])
    return w.done() + struct.pack(">I", zlib.adler32(filtered_frame.tobytes()))


def canonical(lengths):
    """RFC 1951 3.2.2"""
    top = max(lengths)
    count = [0] * (top + 1)
    for l in lengths:
        if l:
            count[l] += 1
    code, nxt = 0, [0] * (top + 1)
    for bits in range(1, top + 1):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for l in lengths:
        out.append(nxt[l] if l else 0)
        if l:
            nxt[l] += 1
    return out


def first_block_type(stream):
    """a zlib stream -> (BFINAL, BTYPE) of its first deflate block"""
    return stream[2] & 1, (stream[2] >> 1) & 3


# ------------------------------------------------------------------------------------------------------------------------------ container
SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOUR_TYPE = {1: 0, 3: 2, 4: 6}


def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def ihdr(W, H, C):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, COLOUR_TYPE[C], 0, 0, 0))


def png_file(W, H, C, stream):
    return SIGNATURE + ihdr(W, H, C) + chunk(b"IDAT", stream) + chunk(b"IEND", b"")


def parse_chunks(data):
    """a PNG / APNG file -> [(kind, body)]; the signature and every CRC are checked"""
    if data[:8] != SIGNATURE:
        raise ValueError("no PNG signature")
    pos, out = 8, []
    while pos < len(data):
        size, kind = struct.unpack_from(">I4s", data, pos)
        body = data[pos + 8:pos + 8 + size]
        if len(body) != size or struct.unpack_from(">I", data, pos + 8 + size)[0] != zlib.crc32(kind + body):
            raise ValueError(f"chunk {kind!r} at byte {pos}: cut short or a wrong CRC")
        out.append((kind, body))
        pos += 12 + size
    return out


def reference_files(frames, filter, strip_rows, deflate_tables):
    """(n, H, W, C) uint8 -> (filtered uint8 (n, H, R), the n files) with deflate_tables (video_io's) building each frame's codes"""
    n, H, W, C = frames.shape
    filtered = filter_frames(frames, filter)
    files = []
    for f in range(n):
        _, hist = tokenize_frame(filtered[f], strip_rows)
        files.append(png_file(W, H, C, zlib_stream(filtered[f], strip_rows, deflate_tables(hist))))
    return filtered, files


def synthetic_portrait(n, H, W, seed):
    """(n, H, W, 3) uint8: a flat background behind a textured oval that moves a little from frame to frame"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((n, H, W, 3), np.uint8)
    for k in range(n):
        inside = ((x - W / 2 - k) / (0.3 * W)) ** 2 + ((y - H / 2) / (0.4 * H)) ** 2 <= 1
        face = np.stack([200 + 20 * np.sin(x / 5), 160 + 15 * np.cos(y / 7), 140 + 10 * np.sin((x + y) / 9)], axis=-1) + rng.normal(0, 2, (H, W, 3))
        out[k] = np.where(inside[..., None], np.clip(face, 0, 255), np.array([32, 96, 160], np.float64)).astype(np.uint8)
    return out
