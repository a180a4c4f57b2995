"""Test infrastructure, not product: a numpy restatement of the layout-aware kernels of emote_hack_amd/csrc/video_in.hip
(emo_jpeg_decode_bits / _decode_segments / _idct / _rgb) for 4:2:0, 4:2:2, 4:4:4 and grey baseline files, in the arithmetic
include/emo_hip.h fixes for them, which is libjpeg's default decoder's.  It builds on tests/jpeg_decode_ref.py - the standard's serial
Huffman decoder (code_tables, _Reader) and the jidctint.c butterfly (_idct_pass) - and has a marker walk of its own, so that nothing here
is shared with emote_hack_amd.video_io.  tests/test_jpeg_layouts_host.py holds it to Pillow's decoder byte for byte; the GPU tests hold
the kernels to it."""
import io

import numpy as np

from tests import jpeg_decode_ref as D
from tests import mjpeg_ref as R

LAYOUTS = {"4:4:4": (3, 1, 1), "4:2:2": (3, 2, 1), "4:2:0": (3, 2, 2), "grey": (1, 1, 1)}      # name -> (components, luminance h, v)
SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}                                            # Pillow's option
# (H, W) per layout: the smallest at which each part can go wrong
SIZES = {"4:2:2": [(8, 5), (8, 16), (17, 33), (38, 70)],          # chroma plane 3 wide, the narrowest that is filtered; one MCU; odd both ways; a grid
         "4:2:0": [(5, 9), (6, 16), (17, 33), (38, 70)],          # tests/jpeg_decode_ref.py's
         "4:4:4": [(1, 1), (8, 8), (9, 4), (16, 3), (17, 33), (38, 70)],      # one pixel; one block; narrower than a block; odd; a grid
         "grey": [(1, 1), (8, 8), (9, 4), (16, 3), (17, 33), (38, 70)]}
QUALITIES = [10, 90, 100]


def bpm(layout):
    nc, hs, vs = layout
    return 1 if nc == 1 else hs * vs + 2


def grid(H, W, layout):
    """(MCU rows, MCU columns): MCUs of 8 h x 8 v pixels; a grey scan is not interleaved, its MCU is a block (T.81 A.2.2)"""
    _, hs, vs = layout
    return -(-H // (8 * vs)), -(-W // (8 * hs))


def pillow_file(picture, name, quality, optimize, **kw):
    """Pillow's baseline file of an (H, W, 3) picture in the layout `name`; grey is saved from the picture's first channel"""
    from PIL import Image
    buf = io.BytesIO()
    if name == "grey":
        Image.fromarray(np.ascontiguousarray(picture[..., 0])).save(buf, format="JPEG", quality=quality, optimize=optimize, **kw)
    else:
        Image.fromarray(picture).save(buf, format="JPEG", quality=quality, subsampling=SUBSAMPLING[name], optimize=optimize, **kw)
    return buf.getvalue()


def three_quantiser_file(picture, name="4:4:4", optimize=False, **kw):
    """a file whose three components use three different quantisation tables (Pillow's qtables=)"""
    tabs = [[min(255, 2 + k + (i % 8) + (i // 8)) for i in range(64)] for k in (0, 5, 11)]
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(picture).save(buf, format="JPEG", qtables=tabs, subsampling=SUBSAMPLING[name], optimize=optimize, **kw)
    return buf.getvalue()


def pillow_decode(data):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)).convert("RGB"))


def split_file(data):
    """a baseline file -> dict: H, W, layout (components, h, v), tq and (td, ta) per component, quant (3, 64) natural per component,
    specs (four (BITS, HUFFVAL): the first component's pair, the last one's), ri (0: none), parts (the unstuffed bytes of every restart
    interval; one for a file without).  The standard's byte-at-a-time rule (B.1.1.5); a walk of its own."""
    quant, huff = R.jpeg_tables_in(data)
    pos, ri = 2, 0
    while True:
        marker, size = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        body = data[pos + 4:pos + 2 + size]
        if marker == 0xC0:
            H, W, nf = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big"), body[5]
            comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(nf)]
        if marker == 0xDD:
            ri = int.from_bytes(body, "big")
        pos += 2 + size
        if marker == 0xDA:
            sel = [(body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(body[0])]
            break
    assert len(sel) == nf and nf in (1, 3)
    layout = (1, 1, 1) if nf == 1 else (3, comps[0][1], comps[0][2])
    assert nf == 1 or all(c[1:3] == (1, 1) for c in comps[1:])
    raw, parts, cur, i = data[pos:], [], bytearray(), 0
    while True:
        if raw[i] != 0xFF:
            cur.append(raw[i])
            i += 1
        elif raw[i + 1] == 0x00:
            cur.append(0xFF)
            i += 2
        else:
            parts.append(np.frombuffer(bytes(cur), np.uint8))
            if not 0xD0 <= raw[i + 1] <= 0xD7:
                break
            cur, i = bytearray(), i + 2
    specs = [huff[(0, sel[0][0])], huff[(1, sel[0][1])], huff[(0, sel[-1][0])], huff[(1, sel[-1][1])]]
    q = np.stack([quant[comps[min(k, nf - 1)][3]] for k in range(3)])
    return dict(H=H, W=W, layout=layout, tq=tuple(c[3] for c in comps), tables=tuple(sel), quant=q, specs=specs, ri=ri, parts=parts)


def huffman_decode(scan, specs, n_mcu, layout):
    """one segment's unstuffed bytes (a whole scan, or a restart interval) -> int16 (n_mcu, bpm, 64), zig-zag order, DC undifferenced
    from predictions 0.  Block k of an MCU belongs to component 0 for k < bpm - 2, then to Cb, then to Cr (T.81 A.2.3).
    D.DecodeError(status) where the kernels report one."""
    tabs = [D.code_tables(*s) for s in specs]
    b = bpm(layout)
    r, pred = D._Reader(scan), [0, 0, 0]
    out = np.zeros((n_mcu, b, 64), np.int16)
    for m in range(n_mcu):
        for k in range(b):
            comp = 0 if b == 1 or k < b - 2 else k - (b - 3)
            dc, ac = (tabs[0], tabs[1]) if comp == 0 else (tabs[2], tabs[3])
            s = r.decode(dc)
            if s > 11:
                raise D.DecodeError(D.BAD_CODE)
            pred[comp] += r.receive_extend(s)
            out[m, k, 0] = pred[comp]
            z = 1
            while z < 64:                                  # figure F.13
                rs = r.decode(ac)
                run, s = rs >> 4, rs & 15
                if s == 0:
                    if rs == 0:
                        break
                    if rs != 0xF0:
                        raise D.DecodeError(D.BAD_CODE)
                    z += 16
                    if z > 64:
                        raise D.DecodeError(D.BAD_RUN)
                    continue
                if s > 10:
                    raise D.DecodeError(D.BAD_CODE)
                v = r.receive_extend(s)
                z += run
                if z > 63:
                    raise D.DecodeError(D.BAD_RUN)
                out[m, k, z] = v
                z += 1
    return out


def coefficients(f):
    """split_file's dict -> int16 (n_mcu, bpm, 64): every restart interval on its own"""
    mr, mc = grid(f["H"], f["W"], f["layout"])
    n_mcu, ri = mr * mc, f["ri"] or mr * mc
    spans = [(m0, min(m0 + ri, n_mcu)) for m0 in range(0, n_mcu, ri)]
    assert len(spans) == len(f["parts"]), (len(spans), len(f["parts"]))
    return np.concatenate([huffman_decode(part, f["specs"], m1 - m0, f["layout"]) for part, (m0, m1) in zip(f["parts"], spans)])


def idct(coefs, quant, H, W, layout):
    """coefficients (n, MCUs, bpm, 64) zig-zag, quant (3, 64) natural, one per component -> (Y uint8 (n, mr * 8 v, mc * 8 h),
    C uint8 (n, 2, mr * 8, mc * 8), or None for grey): the planes padded to whole MCUs"""
    coefs = np.asarray(coefs)
    nc, hs, vs = layout
    n, b, ny = coefs.shape[0], bpm(layout), (1 if nc == 1 else hs * vs)
    mr, mc = grid(H, W, layout)
    nat = np.zeros(coefs.shape, np.int32)
    nat[..., R.ZIGZAG] = coefs.astype(np.int32)
    q = np.asarray(quant, np.int32).reshape(3, 64)
    with np.errstate(over="ignore"):
        nat = nat * np.stack([q[0]] * ny + [q[1], q[2]][:b - ny])[None, None]
    blk = nat.reshape(n, mr * mc, b, 8, 8)
    ws = D._idct_pass(blk.swapaxes(-1, -2), 11).swapaxes(-1, -2)          # columns
    px = np.clip(D._idct_pass(ws, 18).astype(np.int64) + 128, 0, 255).astype(np.uint8)
    px = px.reshape(n, mr, mc, b, 8, 8)
    y = px[:, :, :, :ny].reshape(n, mr, mc, vs, hs, 8, 8).transpose(0, 1, 3, 5, 2, 4, 6).reshape(n, mr * 8 * vs, mc * 8 * hs)
    c = px[:, :, :, ny:].transpose(0, 3, 1, 4, 2, 5).reshape(n, 2, mr * 8, mc * 8) if nc == 3 else None
    return y, c


def to_rgb(y, c, H, W, layout):
    """the planes -> (n, H, W, 3) uint8.  4:2:0: h2v2 fancy up-sampling (D.h2v2_rgb).  4:2:2: h2v1_fancy_upsample on the ceil(W / 2)
    real chroma samples of a row - even columns (3 p + left + 1) >> 2, odd ones (3 p + right + 2) >> 2, neighbours clamped to the plane -
    and no filter down the columns.  4:4:4: chroma as it is.  Then jdcolor.c's fixed-point transform.  Grey: the sample three times."""
    nc, hs, vs = layout
    lum = np.asarray(y)[:, :H, :W].astype(np.int64)
    if nc == 1:
        return np.repeat(lum[..., None], 3, -1).astype(np.uint8)
    if (hs, vs) == (2, 2):
        return D.h2v2_rgb(y, c, H, W)
    if (hs, vs) == (2, 1):
        cw = (W + 1) // 2
        p = np.asarray(c)[:, :, :H, :cw].astype(np.int64)
        left, right = np.concatenate([p[..., :1], p[..., :-1]], -1), np.concatenate([p[..., 1:], p[..., -1:]], -1)
        o = np.stack([(3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2], -1).reshape(p.shape[0], 2, H, 2 * cw)[..., :W]
    else:
        o = np.asarray(c)[:, :, :H, :W].astype(np.int64)
    cb, cr = o[:, 0] - 128, o[:, 1] - 128
    rgb = np.stack([lum + ((91881 * cr + 32768) >> 16), lum + ((-22554 * cb - 46802 * cr + 32768) >> 16), lum + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def decode_all(data):
    """one file -> (split_file's dict, coefficients (n_mcu, bpm, 64), Y plane, C planes or None, RGB (H, W, 3)): every stage of the
    restatement, in the kernels' layouts"""
    f = split_file(data)
    coefs = coefficients(f)
    y, c = idct(coefs[None], f["quant"], f["H"], f["W"], f["layout"])
    rgb = to_rgb(y, c, f["H"], f["W"], f["layout"])[0]
    return f, coefs, y[0], (None if c is None else c[0]), rgb


def decode(data):
    """one file -> (H, W, 3) uint8, the whole restatement"""
    return decode_all(data)[4]
