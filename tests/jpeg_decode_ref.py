"""Test infrastructure, not product: a numpy restatement of the three kernels of emote_hack_amd/csrc/video_in.hip - the arithmetic
include/emo_hip.h fixes for them, which is libjpeg's default decoder's - with the standard's serial Huffman decoder (T.81 F.2.2: DECODE by
MINCODE / MAXCODE / VALPTR one bit at a time, RECEIVE, EXTEND), and a marker walk of its own, so that nothing here is shared with
emote_hack_amd.video_io.  tests/test_jpeg_decode_host.py holds it to Pillow's decoder byte for byte; the GPU tests hold the kernels to it."""
import io

import numpy as np

from tests import mjpeg_ref as R

OK, BAD_CODE, PAST_END, BAD_RUN = 0, 1, 2, 3           # emo_jpeg_decode_bits' status values
PILLOW_SIZES = [(5, 9), (6, 16), (17, 33), (38, 70)]    # (H, W) of the issue's 9x5, 16x6, 33x17 and 70x38
PILLOW_QUALITIES = [10, 90, 100]


class DecodeError(Exception):
    def __init__(self, status):
        super().__init__(status)
        self.status = status


def code_tables(bits, huffval):
    """Annex C + F.2.2.3: (MINCODE, MAXCODE, VALPTR) indexed by code length 1 .. 16 (MAXCODE -1: no code of that length), HUFFVAL"""
    mincode, maxcode, valptr = [0] * 17, [-1] * 17, [0] * 17
    code, k = 0, 0
    for size in range(1, 17):
        if bits[size - 1]:
            valptr[size], mincode[size] = k, code
            code, k = code + bits[size - 1], k + bits[size - 1]
            maxcode[size] = code - 1
        code <<= 1
    return mincode, maxcode, valptr, bytes(huffval)


class _Reader:
    def __init__(self, scan):
        self.bits = np.unpackbits(np.asarray(scan, np.uint8)).tolist()
        self.pos = 0

    def bit(self):
        if self.pos >= len(self.bits):
            raise DecodeError(PAST_END)
        self.pos += 1
        return self.bits[self.pos - 1]

    def decode(self, tab):                                 # figure F.16
        mincode, maxcode, valptr, huffval = tab
        code = self.bit()
        for size in range(1, 17):
            if code <= maxcode[size]:
                return huffval[valptr[size] + code - mincode[size]]
            if size < 16:
                code = code << 1 | self.bit()
        raise DecodeError(BAD_CODE)

    def receive_extend(self, s):                           # figures F.17 and F.12
        v = 0
        for _ in range(s):
            v = v << 1 | self.bit()
        return v - (1 << s) + 1 if s and v < 1 << (s - 1) else v


def huffman_decode(scan, specs, n_mcu):
    """one frame's unstuffed scan, four (BITS, HUFFVAL) in the order DC luma, AC luma, DC chroma, AC chroma -> int16 (n_mcu, 6, 64),
    zig-zag order, DC undifferenced.  DecodeError(status) where emo_jpeg_decode_bits reports one."""
    tabs = [code_tables(*s) for s in specs]
    r, pred = _Reader(scan), [0, 0, 0]
    out = np.zeros((n_mcu, 6, 64), np.int16)
    for m in range(n_mcu):
        for b in range(6):
            comp = 0 if b < 4 else b - 3
            dc, ac = (tabs[0], tabs[1]) if comp == 0 else (tabs[2], tabs[3])
            s = r.decode(dc)
            if s > 11:
                raise DecodeError(BAD_CODE)
            pred[comp] += r.receive_extend(s)
            out[m, b, 0] = pred[comp]
            k = 1
            while k < 64:                                  # figure F.13
                rs = r.decode(ac)
                run, s = rs >> 4, rs & 15
                if s == 0:
                    if rs == 0:
                        break
                    if rs != 0xF0:
                        raise DecodeError(BAD_CODE)
                    k += 16
                    if k > 64:
                        raise DecodeError(BAD_RUN)
                    continue
                if s > 10:
                    raise DecodeError(BAD_CODE)
                v = r.receive_extend(s)
                k += run
                if k > 63:
                    raise DecodeError(BAD_RUN)
                out[m, b, k] = v
                k += 1
    return out


def _idct_pass(x, shift):
    """the 8-point butterfly of jidctint.c along the LAST axis, int32 with wrap-around"""
    i0, i1, i2, i3, i4, i5, i6, i7 = (x[..., k].astype(np.int32) for k in range(8))
    with np.errstate(over="ignore"):
        z1 = (i2 + i6) * np.int32(4433)
        t2, t3 = z1 - i6 * np.int32(15137), z1 + i2 * np.int32(6270)
        t0, t1 = (i0 + i4) * np.int32(8192), (i0 - i4) * np.int32(8192)
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        a0, a1, a2, a3 = i7, i5, i3, i1
        z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
        z5 = (z3 + z4) * np.int32(9633)
        a0, a1, a2, a3 = a0 * np.int32(2446), a1 * np.int32(16819), a2 * np.int32(25172), a3 * np.int32(12299)
        z1, z2 = z1 * np.int32(-7373), z2 * np.int32(-20995)
        z3, z4 = z3 * np.int32(-16069) + z5, z4 * np.int32(-3196) + z5
        a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
        rnd = np.int32(1 << (shift - 1))
        outs = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
        return np.stack([(o + rnd) >> np.int32(shift) for o in outs], axis=-1)


def idct(coefs, quant, H, W):
    """coefficients (n, MCUs, 6, 64) zig-zag, quant (2, 64) natural -> (Y uint8 (n, mr * 16, mc * 16), C uint8 (n, 2, mr * 8, mc * 8))"""
    coefs = np.asarray(coefs)
    n = coefs.shape[0]
    mr, mc = R.n_mcus(H, W)
    nat = np.zeros(coefs.shape, np.int32)
    nat[..., R.ZIGZAG] = coefs.astype(np.int32)
    q = np.asarray(quant, np.int32).reshape(2, 64)
    with np.errstate(over="ignore"):
        nat = nat * np.stack([q[0]] * 4 + [q[1]] * 2)[None, None]
    blk = nat.reshape(n, mr * mc, 6, 8, 8)
    ws = _idct_pass(blk.swapaxes(-1, -2), 11).swapaxes(-1, -2)          # columns
    px = np.clip(_idct_pass(ws, 18).astype(np.int64) + 128, 0, 255).astype(np.uint8)
    px = px.reshape(n, mr, mc, 6, 8, 8)
    y = px[:, :, :, :4].reshape(n, mr, mc, 2, 2, 8, 8).transpose(0, 1, 3, 5, 2, 4, 6).reshape(n, mr * 16, mc * 16)
    c = px[:, :, :, 4:].transpose(0, 3, 1, 4, 2, 5).reshape(n, 2, mr * 8, mc * 8)
    return y, c


def h2v2_rgb(y, c, H, W):
    """the planes -> (n, H, W, 3) uint8: h2v2 fancy up-sampling on the real chroma plane, then the fixed-point colour transform"""
    ch, cw = (H + 1) // 2, (W + 1) // 2
    p = np.asarray(c)[:, :, :ch, :cw].astype(np.int64)
    up, down = np.concatenate([p[:, :, :1], p[:, :, :-1]], 2), np.concatenate([p[:, :, 1:], p[:, :, -1:]], 2)
    s = np.stack([3 * p + up, 3 * p + down], 3).reshape(p.shape[0], 2, 2 * ch, cw)
    left, right = np.concatenate([s[..., :1], s[..., :-1]], -1), np.concatenate([s[..., 1:], s[..., -1:]], -1)
    o = np.stack([(3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4], -1).reshape(p.shape[0], 2, 2 * ch, 2 * cw)[:, :, :H, :W]
    lum = np.asarray(y)[:, :H, :W].astype(np.int64)
    cb, cr = o[:, 0] - 128, o[:, 1] - 128
    rgb = np.stack([lum + ((91881 * cr + 32768) >> 16), lum + ((-22554 * cb - 46802 * cr + 32768) >> 16), lum + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def split_file(data):
    """a baseline 4:2:0 file -> (H, W, quant (2, 64) natural, four (BITS, HUFFVAL), unstuffed scan uint8); a walk of its own"""
    quant, huff = R.jpeg_tables_in(data)
    pos = 2
    while True:
        marker, size = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        if marker == 0xC0:
            H, W = int.from_bytes(data[pos + 5:pos + 7], "big"), int.from_bytes(data[pos + 7:pos + 9], "big")
            assert data[pos + 9] == 3 and bytes(data[pos + 10:pos + 19:3]) == b"\x01\x02\x03" and data[pos + 11] == 0x22
            tq = [data[pos + 12], data[pos + 15]]
        pos += 2 + size
        if marker == 0xDA:
            break
    raw, scan, i = data[pos:], bytearray(), 0
    while not (raw[i] == 0xFF and raw[i + 1] != 0):         # the standard's byte-at-a-time rule (B.1.1.5)
        scan.append(raw[i])
        i += 2 if raw[i] == 0xFF else 1
    specs = [huff[(0, 0)], huff[(1, 0)], huff[(0, 1)], huff[(1, 1)]]
    return H, W, np.stack([quant[tq[0]], quant[tq[1]]]), specs, np.frombuffer(bytes(scan), np.uint8)


def decode(data):
    """one file -> (H, W, 3) uint8, the whole restatement"""
    H, W, quant, specs, scan = split_file(data)
    mr, mc = R.n_mcus(H, W)
    coefs = huffman_decode(scan, specs, mr * mc)[None]
    return h2v2_rgb(*idct(coefs, quant, H, W), H, W)[0]


def pillow_file(frame, quality, optimize):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG", quality=quality, subsampling=2, optimize=optimize)
    return buf.getvalue()


def picture(H, W, seed):
    """an (H, W, 3) uint8 frame with edges, texture and saturated patches, the same every call"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    f = np.stack([255.0 * x / max(W - 1, 1), 255.0 * y / max(H - 1, 1), 128 + 100 * np.sin(x / 3.0) * np.cos(y / 2.0)], -1) + rng.normal(0, 12, (H, W, 3))
    f[: H // 3, : W // 3] = (255, 0, 0)
    f[H // 2:, W // 2:] = rng.integers(0, 256, (H - H // 2, W - W // 2, 3))
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)
