"""What the GIF tests measure against, in numpy and plain Python, independent of emote_hack_amd: the synthetic clip, the brute-force nearest
palette entry, the Bayer matrix from its recursion, a GIF89a parser with an LZW decoder of its own (so a stream is checked twice: by it
and by Pillow), and a serial strip-wise LZW encoder that models the DECODER's table to find every code's width (the kernels use a closed
form of the code's index instead).  The encoder feeds the host framing test and is compared with the device's streams byte for byte."""
import struct

import numpy as np

CLEAR, EOI, FIRST_FREE, TABLE_MAX = 256, 257, 258, 4096


def synthetic_clip(n, H, W, seed):
    """(n, H, W, 3) uint8: smooth waves and ramps with N(0, 6) noise, and a flat, slightly noisy rectangle (a face-coloured patch)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((n, H, W, 3), np.float64)
    for k in range(n):
        out[k, ..., 0] = 128 + 100 * np.sin(x / (9 + k) + y / 17)
        out[k, ..., 1] = 128 + 90 * np.cos(y / 11 - 0.3 * k)
        out[k, ..., 2] = 0.6 * 255 * x / W + 0.4 * 255 * y / H
    out += rng.normal(0, 6, out.shape)
    patch = out[:, H // 4:H // 2, W // 4:W // 2]
    patch[...] = np.array([230, 180, 150], np.float64) + rng.normal(0, 3, patch.shape)
    return np.clip(out, 0, 255).astype(np.uint8)


def histogram(frames):
    """(..., 3) uint8 -> int64 (32768, 4): count and sums of R, G, B per bin (r >> 3, g >> 3, b >> 3), by np.bincount"""
    px = frames.reshape(-1, 3).astype(np.int64)
    bins = ((px[:, 0] >> 3) << 10) | ((px[:, 1] >> 3) << 5) | (px[:, 2] >> 3)
    # weights make bincount sum in float64: exact here, the tests' sums stay far below 2^53
    cols = [np.bincount(bins, minlength=32768)] + [np.bincount(bins, weights=px[:, c], minlength=32768) for c in range(3)]
    return np.stack(cols, axis=1).astype(np.int64)


def nearest(pixels, palette):
    """(..., 3) uint8 pixels, (k, 3) uint8 palette -> uint8 (...): argmin of the squared distance in int64; argmin keeps the first minimum"""
    px = pixels.reshape(-1, 1, 3).astype(np.int64)
    pal = palette.reshape(1, -1, 3).astype(np.int64)
    out = np.empty(px.shape[0], np.uint8)
    for at in range(0, px.shape[0], 4096):
        d = ((px[at:at + 4096] - pal) ** 2).sum(axis=2)
        out[at:at + 4096] = np.argmin(d, axis=1)
    return out.reshape(pixels.shape[:-1])


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def bayer(size):
    """B1 = [[0]], B2k = [[4B, 4B + 2], [4B + 3, 4B + 1]]"""
    b = np.zeros((1, 1), np.int64)
    while b.shape[0] < size:
        b = np.block([[4 * b, 4 * b + 2], [4 * b + 3, 4 * b + 1]])
    return b


def dithered(frames, strength):
    """clamp(v + floor((2 B8[y & 7][x & 7] - 63) * strength / 128), 0, 255) on every channel of (n, H, W, 3) uint8 frames"""
    n, H, W, _ = frames.shape
    b8 = bayer(8)
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.floor_divide((2 * b8[yy & 7, xx & 7] - 63) * int(strength), 128)
    return np.clip(frames.astype(np.int64) + d[None, :, :, None], 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------------------ LZW
class _BitWriter:
    def __init__(self):
        self.out, self.acc, self.n, self.bits = bytearray(), 0, 0, 0

    def put(self, code, width):
        self.acc |= code << self.n
        self.n += width
        self.bits += width
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out), self.bits


def lzw_encode_strips(indices, strip_rows=None):
    """(H, W) uint8 palette indices -> (bytes, bits): GIF89a Appendix F at code size 8, the frame cut into strips of strip_rows rows (None:
    one).  The first strip opens with Clear; every strip starts from an empty dictionary and ends with Clear, the last with End of
    Information; a full table (4096) is followed by Clear.  Every code is written at the width a DECODER holds when it reads it: the
    decoder adds an entry per code behind the first after a Clear and widens when its next free code reaches 1 << width."""
    H, W = indices.shape
    rows = H if strip_rows is None else int(strip_rows)
    w = _BitWriter()
    state = dict(width=9, next=FIRST_FREE, prev=False)

    def emit(code):
        w.put(code, state["width"])
        if code == CLEAR:
            state.update(width=9, next=FIRST_FREE, prev=False)
            return
        if state["prev"] and state["next"] < TABLE_MAX:
            state["next"] += 1
            if state["next"] == 1 << state["width"] and state["width"] < 12:
                state["width"] += 1
        state["prev"] = True

    emit(CLEAR)
    starts = list(range(0, H, rows))
    for r0 in starts:
        table, free, cur = {}, FIRST_FREE, None
        for k in indices[r0:r0 + rows].reshape(-1).tolist():
            if cur is None:
                cur = k
            elif (cur, k) in table:
                cur = table[cur, k]
            else:
                emit(cur)
                if free < TABLE_MAX:
                    table[cur, k] = free
                    free += 1
                else:
                    emit(CLEAR)
                    table, free = {}, FIRST_FREE
                cur = k
        emit(cur)
        emit(EOI if r0 == starts[-1] else CLEAR)
    return w.done()


def lzw_decode(data, n_pixels):
    """the image data of one frame (sub-blocks joined) -> n_pixels indices as bytes; ValueError for a stream that is not valid or not
    complete.  Table entries as byte strings: simple, and fast enough for the tests' frames."""
    table = [bytes([i]) for i in range(CLEAR)] + [b"", b""]
    width, prev, out = 9, None, bytearray()
    acc = nbits = pos = 0
    while True:
        while nbits < width:
            if pos >= len(data):
                raise ValueError(f"the stream ends after {len(out)} of {n_pixels} pixels without End of Information")
            acc |= data[pos] << nbits
            nbits += 8
            pos += 1
        code = acc & ((1 << width) - 1)
        acc >>= width
        nbits -= width
        if code == CLEAR:
            del table[FIRST_FREE:]
            width, prev = 9, None
            continue
        if code == EOI:
            break
        if prev is None:
            if code >= CLEAR:
                raise ValueError(f"code {code} right behind a Clear")
            entry = table[code]
        else:
            if code < len(table):
                entry = table[code]
            elif code == len(table) and len(table) < TABLE_MAX:
                entry = prev + prev[:1]
            else:
                raise ValueError(f"code {code} with {len(table)} entries in the table")
            if len(table) < TABLE_MAX:
                table.append(prev + entry[:1])
                if len(table) == 1 << width and width < 12:
                    width += 1
        out += entry
        prev = entry
    if len(out) != n_pixels:
        raise ValueError(f"{len(out)} pixels decoded, the frame has {n_pixels}")
    if pos != len(data):
        raise ValueError(f"{len(data) - pos} bytes behind End of Information")
    return bytes(out)


# ------------------------------------------------------------------------------------------------------------------------------ container
def parse_gif(data):
    """a GIF89a file -> dict(width, height, global_table (k, 3) uint8 | None, loop int | None, frames: list of dict(delay, disposal,
    transparent, left, top, width, height, table | None, code_size, sub_blocks: list of sizes, indices (h, w) uint8), trailer bool)"""
    if data[:6] != b"GIF89a":
        raise ValueError("no GIF89a header")
    width, height, flags, _, _ = struct.unpack_from("<HHBBB", data, 6)
    pos, out = 13, dict(width=width, height=height, global_table=None, loop=None, frames=[], trailer=False)
    if flags & 0x80:
        k = 2 << (flags & 7)
        out["global_table"] = np.frombuffer(data, np.uint8, 3 * k, pos).reshape(k, 3)
        pos += 3 * k
    control = None

    def blocks(pos):
        sizes, body = [], bytearray()
        while True:
            size = data[pos]
            pos += 1
            if size == 0:
                return sizes, bytes(body), pos
            sizes.append(size)
            body += data[pos:pos + size]
            if pos + size > len(data):
                raise ValueError("a sub-block runs past the end of the file")
            pos += size

    while pos < len(data):
        kind = data[pos]
        pos += 1
        if kind == 0x3B:
            out["trailer"] = True
            if pos != len(data):
                raise ValueError("bytes behind the trailer")
            break
        if kind == 0x21:
            label = data[pos]
            sizes, body, pos = blocks(pos + 1)
            if label == 0xF9:
                if sizes != [4]:
                    raise ValueError("a malformed graphic control extension")
                packed, delay, transparent = struct.unpack("<BHB", body)
                control = dict(delay=delay, disposal=(packed >> 2) & 7, transparent=transparent if packed & 1 else None)
            elif label == 0xFF and body[:11] == b"NETSCAPE2.0":
                if sizes != [11, 3] or body[11] != 1:
                    raise ValueError("a malformed NETSCAPE2.0 extension")
                out["loop"] = struct.unpack_from("<H", body, 12)[0]
        elif kind == 0x2C:
            left, top, w, h, packed = struct.unpack_from("<HHHHB", data, pos)
            pos += 9
            table = None
            if packed & 0x80:
                k = 2 << (packed & 7)
                table = np.frombuffer(data, np.uint8, 3 * k, pos).reshape(k, 3)
                pos += 3 * k
            if packed & 0x40:
                raise ValueError("an interlaced frame")
            code_size = data[pos]
            sizes, body, pos = blocks(pos + 1)
            if code_size != 8:
                raise ValueError(f"code size {code_size}")
            frame = dict(control or dict(delay=None, disposal=None, transparent=None))
            frame.update(left=left, top=top, width=w, height=h, table=table, code_size=code_size, sub_blocks=sizes, stream=body,
                         indices=np.frombuffer(lzw_decode(body, w * h), np.uint8).reshape(h, w))
            out["frames"].append(frame)
            control = None
        else:
            raise ValueError(f"block {kind:#04x} at byte {pos - 1}")
    return out
