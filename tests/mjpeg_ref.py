"""Test infrastructure, not product: a float64 numpy restatement of the three kernels of emote_hack_amd/csrc/video_out.hip, written from
ITU-T T.81 (A.3.3 FDCT, A.3.4 quantisation, figure A.6 zig-zag, F.1.2 Huffman coding) and from the arithmetic include/emo_hip.h fixes, plus
the frames the Motion-JPEG tests share.  The entropy coder is the standard's serial procedure (a run counter walked along the zig-zag
sequence), not the kernels' ballot-and-prefix-sum form."""
import io

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
_u, _x = np.arange(8)[:, None], np.arange(8)[None, :]
DCT = 0.5 * np.where(_u == 0, 1.0 / np.sqrt(2.0), 1.0) * np.cos((2 * _x + 1) * _u * np.pi / 16.0)      # C[u][x], A.3.3

SHAPES = [(1, 16, 16), (1, 8, 8), (2, 24, 40), (3, 70, 38)]      # one MCU; smaller than an MCU; half MCUs both ways; a grid size, odd tails
CONTENTS = ["flat", "ramp", "noise", "impulses"]
QUALITIES = [10, 50, 90, 100]


def make_frames(content, n, H, W):
    """(n, H, W, 3) uint8, the same every call"""
    rng = np.random.default_rng(1000 * CONTENTS.index(content) + 100 * n + H + W)
    if content == "flat":                                  # EOB-only AC, zero DC differences (also across MCUs)
        f = np.empty((n, H, W, 3), np.uint8)
        f[:] = (200, 90, 40)
        return f
    if content == "ramp":                                  # a smooth ramp with mild noise; every frame another slope
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        out = []
        for i in range(n):
            base = np.stack([255.0 * x / max(W - 1, 1), 255.0 * y / max(H - 1, 1), 255.0 * (x + y) / max(W + H - 2, 1)], -1)
            out.append(np.roll(base, i, axis=-1) * 0.8 + 20.0 + rng.normal(0.0, 3.0, (H, W, 3)))
        return np.clip(np.rint(np.stack(out)), 0, 255).astype(np.uint8)
    if content == "noise":
        # full range at both scales: every pixel independent, and over it 8x8 cells (on the block grid) of solid black, solid white or a
        # black | white split - a black block beside a white one is a DC difference of 2040 (category 11), a split block an AC term of
        # 924 (category 10); independent pixels alone stay two categories below both
        f = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
        for i in range(n):
            for y0 in range(0, H, 8):
                for x0 in range(0, W, 8):
                    kind = int(rng.integers(0, 6))
                    if kind < 3:
                        f[i, y0:y0 + 8, x0:x0 + 8] = (0, 255, 0)[kind]
                        if kind == 2:
                            f[i, y0:y0 + 8, x0 + 4:x0 + 8] = 255
        return f
    if content == "impulses":                              # a mid-grey field with a few isolated saturated pixels
        f = np.full((n, H, W, 3), 128, np.uint8)
        k = max(1, (n * H * W) // 48)
        idx = rng.choice(n * H * W, size=k, replace=False)
        f.reshape(-1, 3)[idx] = rng.choice(np.array([0, 255], np.uint8), size=(k, 3))
        return f
    raise ValueError(content)


def n_mcus(H, W):
    return (-(-H // 16)), (-(-W // 16))


def blocks(frames, quant):
    """frames uint8 (n, H, W, 3), quant (2, 64) natural order -> (coefficients int16 (n, MCUs, 6, 64) zig-zag order with the DC
    undifferenced, the float64 quotients S / q they were rounded from)"""
    n, H, W, _ = frames.shape
    mr, mc = n_mcus(H, W)
    p = np.pad(frames.astype(np.float64), ((0, 0), (0, mr * 16 - H), (0, mc * 16 - W), (0, 0)), mode="edge")
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b - 128.0
    cb = -0.168736 * r - 0.331264 * g + 0.5 * b
    cr = 0.5 * r - 0.418688 * g - 0.081312 * b
    sub = lambda c: c.reshape(n, mr * 8, 2, mc * 8, 2).mean(axis=(2, 4))
    yb = y.reshape(n, mr, 2, 8, mc, 2, 8).transpose(0, 1, 4, 2, 5, 3, 6).reshape(n, mr, mc, 4, 8, 8)
    cbb, crb = (sub(c).reshape(n, mr, 8, mc, 8).transpose(0, 1, 3, 2, 4)[:, :, :, None] for c in (cb, cr))
    s = np.concatenate([yb, cbb, crb], axis=3).reshape(n, mr * mc, 6, 8, 8)
    S = np.einsum("vy,nmbyx,ux->nmbvu", DCT, s, DCT).reshape(n, mr * mc, 6, 64)
    q = np.asarray(quant, np.float64).reshape(2, 64)
    quot = S / np.stack([q[0]] * 4 + [q[1]] * 2)[None, None]
    quot = quot[..., ZIGZAG]
    return np.rint(quot).astype(np.int16), quot


def _category(v):
    return int(abs(int(v))).bit_length()


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc, self.n = (self.acc << length) | code, self.n + length

    def bytes(self):
        pad = -self.n % 8
        return np.frombuffer((self.acc << pad).to_bytes((self.n + pad) // 8, "big"), np.uint8)


def entropy(coefs, huff):
    """coefficients (n, MCUs, 6, 64), huff uint32 (4, 256) = length << 16 | code (DC luma, AC luma, DC chroma, AC chroma) -> (bit counts
    int32 (n, MCUs * 6), [(the frame's unstuffed stream as uint8 with zero bits behind the last, its bits)], what was coded: the largest DC
    and AC categories and the number of ZRL codes)"""
    coefs = np.asarray(coefs)
    n, m = coefs.shape[:2]
    code, length = np.asarray(huff, np.int64) & 0xFFFF, np.asarray(huff, np.int64) >> 16
    counts, streams = np.zeros((n, m * 6), np.int32), []
    seen = dict(dc_category=0, ac_category=0, zrl=0, eob=0)
    for f in range(n):
        w, pred = _Bits(), [0, 0, 0]                     # F.1.1.5.1: the predictions start at 0 with the scan (one scan per frame)
        for blk in range(m * 6):
            start = w.n
            comp = 0 if blk % 6 < 4 else blk % 6 - 3
            dc, ac = (0, 1) if comp == 0 else (2, 3)
            zz = [int(v) for v in coefs[f, blk // 6, blk % 6]]
            diff, pred[comp] = zz[0] - pred[comp], zz[0]
            put_value = lambda tab, sym, v, ssss: (w.put(int(code[tab, sym]), int(length[tab, sym])),
                                                   w.put((v if v >= 0 else v - 1) & ((1 << ssss) - 1), ssss))
            ssss = _category(diff)
            assert length[dc, ssss] > 0
            put_value(dc, ssss, diff, ssss)
            seen["dc_category"] = max(seen["dc_category"], ssss)
            run = 0
            for k in range(1, 64):                       # figure F.2
                if zz[k] == 0:
                    run += 1
                    continue
                while run > 15:
                    w.put(int(code[ac, 0xF0]), int(length[ac, 0xF0]))
                    run -= 16
                    seen["zrl"] += 1
                ssss = _category(zz[k])
                assert length[ac, run << 4 | ssss] > 0
                put_value(ac, run << 4 | ssss, zz[k], ssss)
                seen["ac_category"] = max(seen["ac_category"], ssss)
                run = 0
            if run:
                w.put(int(code[ac, 0]), int(length[ac, 0]))
                seen["eob"] += 1
            counts[f, blk] = w.n - start
        streams.append((w.bytes(), w.n))
    return counts, streams, seen


def jpeg_tables_in(data):
    """the tables a JPEG file carries, parsed from its bytes: ({Tq: 64 entries in NATURAL order}, {(Tc, Th): (BITS tuple, HUFFVAL bytes)})"""
    assert data[:2] == b"\xFF\xD8"
    pos, quant, huff = 2, {}, {}
    while True:
        assert data[pos] == 0xFF, pos
        marker, size = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        body = data[pos + 4:pos + 2 + size]
        if marker == 0xDB:                                # B.2.4.1: Pq | Tq, then 64 entries in zig-zag order
            while body:
                assert body[0] >> 4 == 0
                nat = np.zeros(64, np.int64)
                nat[ZIGZAG] = np.frombuffer(body[1:65], np.uint8)
                quant[body[0] & 15], body = nat, body[65:]
        elif marker == 0xC4:                              # B.2.4.2: Tc | Th, BITS, HUFFVAL
            while body:
                bits = tuple(body[1:17])
                huff[(body[0] >> 4, body[0] & 15)], body = (bits, bytes(body[17:17 + sum(bits)])), body[17 + sum(bits):]
        elif marker == 0xDA:
            return quant, huff
        pos += 2 + size


def psnr(a, b):
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


def pillow_jpeg(frame, quality):
    """Pillow's own baseline file of one (H, W, 3) frame: 4:2:0, the standard Huffman tables"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG", quality=quality, subsampling=2, optimize=False)
    return buf.getvalue()


def decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im.convert("RGB"))
