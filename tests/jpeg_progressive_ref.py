"""Test infrastructure, not product: progressive JPEG (T.81 Annex G, SOF2, Huffman coding) for the tests of emo_jpeg_progressive_scan
and of parse_jpeg / decode_mjpeg(progressive=True).  Three parts, none of which shares code with emote_hack_amd.video_io or the kernel:
  - pillow_progressive: Pillow's own writer, which gives libjpeg's default script (10 scans in colour, 6 in grey, spectral selection and
    successive approximation both);
  - split_progressive / decode_coefficients: a marker walk and a serial decoder written from T.81 G.1.2 (figures G.3 - G.7 read as
    decoding procedures, G.2), into the coefficient buffer (n_mcu, bpm, 64) the emo_jpeg_idct entry reads;
  - write_progressive: a writer that codes such a buffer under a GIVEN script, with fixed canonical Huffman tables (size does not matter
    here), because Pillow cannot choose scripts.
tests/test_jpeg_progressive_host.py holds the decoder (plus the IDCT and colour restatements of tests/jpeg_layout_ref.py) to Pillow byte
for byte, on Pillow's files and on the writer's; the GPU tests hold the kernel to the decoder."""
import io

import numpy as np

from tests import jpeg_decode_ref as D
from tests import jpeg_layout_ref as L
from tests import mjpeg_ref as R

# (H, W): one block; luminance scans walk 3 x 2 blocks inside 4 x 2 at 4:2:0; the narrowest width halved chroma takes; the siblings' size
SIZES = [(8, 8), (9, 17), (33, 5), (38, 70)]
QUALITIES = [10, 90, 100]       # long EOB runs; the usual; dense refinement with many correction bits
FLAT = (128, 136)               # a flat 4:4:4 frame of 272 blocks per component: EOBRUN passes 255


def pillow_progressive(picture, name, quality, **restart):
    """Pillow's progressive file of an (H, W, 3) picture in the layout `name` (a key of L.LAYOUTS; grey from the first channel);
    restart: restart_marker_rows= / restart_marker_blocks="""
    return L.pillow_file(picture, name, quality, True, progressive=True, **restart)


def flat_picture():
    p = np.empty(FLAT + (3,), np.uint8)
    p[:] = (200, 90, 30)
    return p


# ------------------------------------------------------------------------------------------------------------------ geometry
def scan_blocks(H, W, layout, comps):
    """the blocks of one scan in coding order, as (MCU, block of the MCU, component): interleaved over all components MCU by MCU
    (A.2.3); one component: its own ceil(ceil(W h / hs) / 8) x ceil(ceil(H v / vs) / 8) blocks in raster order (A.2.2)"""
    nc, hs, vs = layout
    b, (mr, mc) = L.bpm(layout), L.grid(H, W, layout)
    comp_of = [0] * (b - 2) + [1, 2] if nc == 3 else [0]
    if len(comps) == nc:
        return [(m, k, comp_of[k]) for m in range(mr * mc) for k in range(b)]
    (c,) = comps
    h, v = (hs, vs) if c == 0 else (1, 1)
    bw, bh = -(-(-(-W * h // hs)) // 8), -(-(-(-H * v // vs)) // 8)
    if c == 0:
        return [((by // vs) * mc + bx // hs, (by % vs) * hs + bx % hs, 0) for by in range(bh) for bx in range(bw)]
    return [(by * mc + bx, hs * vs + c - 1, c) for by in range(bh) for bx in range(bw)]


def units_of(H, W, layout, comps):
    """restart intervals count units: MCUs of an interleaved scan, blocks of a one-component scan"""
    return len(scan_blocks(H, W, layout, comps)) // (L.bpm(layout) if len(comps) == layout[0] else 1)


# ------------------------------------------------------------------------------------------------------------------ the walk
def split_progressive(data):
    """a progressive file -> dict: H, W, layout, quant (3, 64) natural per component, scans: a list of dicts comps (indices), Ss, Se, Ah,
    Al, tables ((td, ta) per component), huff (the DHT state AT that scan, {(class, destination): (BITS, HUFFVAL)}), ri, parts (the
    unstuffed bytes of every restart interval).  Byte at a time (B.1.1.5)."""
    pos, ri, quant, huff, scans = 2, 0, {}, {}, []
    while True:
        assert data[pos] == 0xFF, pos
        marker = data[pos + 1]
        if marker == 0xD9:
            break
        size = int.from_bytes(data[pos + 2:pos + 4], "big")
        body = data[pos + 4:pos + 2 + size]
        pos += 2 + size
        if marker == 0xDB:
            while body:
                assert body[0] >> 4 == 0
                nat = np.zeros(64, np.uint16)
                nat[R.ZIGZAG] = np.frombuffer(body[1:65], np.uint8)
                quant[body[0] & 15], body = nat, body[65:]
        elif marker == 0xC4:
            while body:
                n = sum(body[1:17])
                huff[(body[0] >> 4, body[0] & 15)], body = (tuple(body[1:17]), bytes(body[17:17 + n])), body[17 + n:]
        elif marker == 0xC2:
            H, W, nf = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big"), body[5]
            comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(nf)]
        elif marker == 0xDD:
            ri = int.from_bytes(body, "big")
        elif marker == 0xDA:
            ns = body[0]
            ids = [c[0] for c in comps]
            sc = dict(comps=tuple(ids.index(body[1 + 2 * i]) for i in range(ns)), tables=tuple((body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(ns)),
                      Ss=body[1 + 2 * ns], Se=body[2 + 2 * ns], Ah=body[3 + 2 * ns] >> 4, Al=body[3 + 2 * ns] & 15, huff=dict(huff), ri=ri, parts=[])
            cur = bytearray()
            while True:
                if data[pos] != 0xFF:
                    cur.append(data[pos])
                    pos += 1
                elif data[pos + 1] == 0x00:
                    cur.append(0xFF)
                    pos += 2
                else:
                    sc["parts"].append(np.frombuffer(bytes(cur), np.uint8))
                    if not 0xD0 <= data[pos + 1] <= 0xD7:
                        break
                    cur, pos = bytearray(), pos + 2
            scans.append(sc)
    layout = (1, 1, 1) if nf == 1 else (3, comps[0][1], comps[0][2])
    q = np.stack([quant[comps[min(k, nf - 1)][3]] for k in range(3)])
    return dict(H=H, W=W, layout=layout, quant=q, scans=scans)


# ------------------------------------------------------------------------------------------------------------------ the decoder
def _correct(r, blk, k, Al):
    """G.1.2.3: one correction bit for a coefficient with a nonzero history, added towards its sign where the bit is not yet set"""
    if r.bit() and not (abs(blk[k]) >> Al) & 1:
        blk[k] += (1 << Al) if blk[k] > 0 else -(1 << Al)


def decode_scan(coefs, f, sc):
    """one scan, all of its restart intervals, into coefs int (n_mcu, bpm, 64) in place.  D.DecodeError(status) where the kernel reports
    one."""
    H, W, layout = f["H"], f["W"], f["layout"]
    blocks = scan_blocks(H, W, layout, sc["comps"])
    per_unit = L.bpm(layout) if len(sc["comps"]) == layout[0] else 1
    units = len(blocks) // per_unit
    ri = sc["ri"] or units
    Ss, Se, Ah, Al = sc["Ss"], sc["Se"], sc["Ah"], sc["Al"]
    tab = {}
    for c, (td, ta) in zip(sc["comps"], sc["tables"]):
        if not (Ss == 0 and Ah):
            tab[c] = D.code_tables(*sc["huff"][(0, td) if Ss == 0 else (1, ta)])
    assert len(sc["parts"]) == -(-units // ri), (len(sc["parts"]), units, ri)
    for i, part in enumerate(sc["parts"]):
        r, pred, eobrun = D._Reader(part), [0, 0, 0], 0
        mine = blocks[i * ri * per_unit:min((i + 1) * ri, units) * per_unit]
        for j, (m, k, c) in enumerate(mine):
            blk = coefs[m, k]
            if Ss == 0 and Ah == 0:                          # G.1.2.1: F.2.2.1 on the point-transformed value
                s = r.decode(tab[c])
                if s > 11:
                    raise D.DecodeError(D.BAD_CODE)
                pred[c] += r.receive_extend(s)
                blk[0] = pred[c] * (1 << Al)
            elif Ss == 0:                                    # G.1.2.1: one bit of precision more
                if r.bit():
                    blk[0] |= 1 << Al
            elif Ah == 0:                                    # G.1.2.2, figures G.3 - G.6 read backwards
                if eobrun:
                    eobrun -= 1
                    continue
                z = Ss
                while z <= Se:
                    rs = r.decode(tab[c])
                    run, s = rs >> 4, rs & 15
                    if s == 0:
                        if run == 15:
                            z += 16
                            if z > Se + 1:
                                raise D.DecodeError(D.BAD_RUN)
                            continue
                        eobrun = (1 << run) + sum(r.bit() << (run - 1 - t) for t in range(run))
                        if eobrun > len(mine) - j:
                            raise D.DecodeError(D.BAD_RUN)
                        eobrun -= 1
                        break
                    if s > 10:
                        raise D.DecodeError(D.BAD_CODE)
                    v = r.receive_extend(s)
                    z += run
                    if z > Se:
                        raise D.DecodeError(D.BAD_RUN)
                    blk[z] = v * (1 << Al)
                    z += 1
            else:                                            # G.1.2.3, figure G.7 read backwards
                z = Ss
                if eobrun == 0:
                    while z <= Se:
                        rs = r.decode(tab[c])
                        run, s = rs >> 4, rs & 15
                        val = 0
                        if s == 1:
                            val = (1 << Al) if r.bit() else -(1 << Al)
                        elif s != 0:
                            raise D.DecodeError(D.BAD_CODE)
                        elif run < 15:
                            eobrun = (1 << run) + sum(r.bit() << (run - 1 - t) for t in range(run))
                            if eobrun > len(mine) - j:
                                raise D.DecodeError(D.BAD_RUN)
                            break
                        while True:                          # `run` coefficients with a zero history are passed, the next one is the place
                            if z > Se:
                                raise D.DecodeError(D.BAD_RUN)
                            if blk[z] != 0:
                                _correct(r, blk, z, Al)
                            elif run == 0:
                                break
                            else:
                                run -= 1
                            z += 1
                        if val:
                            blk[z] = val
                        z += 1
                if eobrun:
                    while z <= Se:
                        if blk[z] != 0:
                            _correct(r, blk, z, Al)
                        z += 1
                    eobrun -= 1


def decode_coefficients(f, scans=None):
    """split_progressive's dict -> int16 (n_mcu, bpm, 64), zig-zag order: every scan (or the first `scans` of them) in file order"""
    mr, mc = L.grid(f["H"], f["W"], f["layout"])
    coefs = np.zeros((mr * mc, L.bpm(f["layout"]), 64), np.int64)
    for sc in f["scans"][:scans]:
        decode_scan(coefs, f, sc)
    return coefs.astype(np.int16)


def decode(data):
    """one progressive file -> (H, W, 3) uint8: the decoder above, then the IDCT and colour restatements of the baseline path"""
    f = split_progressive(data)
    y, c = L.idct(decode_coefficients(f)[None], f["quant"], f["H"], f["W"], f["layout"])
    return L.to_rgb(y, c, f["H"], f["W"], f["layout"])[0]


# ------------------------------------------------------------------------------------------------------------------ the writer
def _canonical(order, lengths):
    """(BITS, HUFFVAL) that gives the symbols of `order` the code lengths `lengths` (non-decreasing)"""
    bits = [0] * 16
    for n in lengths:
        bits[n - 1] += 1
    return tuple(bits), bytes(order)


# fixed, valid tables: a DC table may hold symbols 0 .. 15 only (libjpeg checks), 16 codes of 5 bits; an AC table all 256 symbols, 255
# codes of 9 bits and one of 10.  A, B, C differ in which symbol gets which code.
TABLES = {"dcA": _canonical(list(range(16)), [5] * 16), "dcB": _canonical(list(range(15, -1, -1)), [5] * 16),
          "dcC": _canonical([(i + 5) % 16 for i in range(16)], [5] * 16),
          "acA": _canonical(list(range(256)), [9] * 255 + [10]), "acB": _canonical(list(range(255, -1, -1)), [9] * 255 + [10]),
          "acC": _canonical([(i + 37) % 256 for i in range(256)], [9] * 255 + [10])}


def _codes(spec):
    bits, vals = spec
    out, code, k = {}, 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            out[vals[k]] = (code, n)
            code, k = code + 1, k + 1
        code <<= 1
    return out


class _Bits:
    def __init__(self):
        self.bits = []

    def put(self, value, n):
        self.bits.extend((value >> (n - 1 - i)) & 1 for i in range(n))

    def bytes(self):
        """padded with 1-bits to a byte (F.1.2.3), stuffed (B.1.1.5)"""
        b = self.bits + [1] * (-len(self.bits) % 8)
        raw = np.packbits(np.array(b, np.uint8)).tobytes() if b else b""
        return raw.replace(b"\xFF", b"\xFF\x00")


def _encode_interval(blocks, coefs, sc, codes):
    """the blocks (MCU, block, component) of one restart interval of scan sc -> its stuffed bytes; jcphuff.c's four encoders"""
    Ss, Se, Ah, Al = sc["Ss"], sc["Se"], sc["Ah"], sc["Al"]
    out, pred = _Bits(), [0, 0, 0]
    eobrun, pending = 0, []                                  # the EOB run and the correction bits that wait behind it

    def flush_eobrun(code):
        nonlocal eobrun, pending
        if eobrun:
            n = eobrun.bit_length() - 1
            out.put(*code[n << 4])
            out.put(eobrun & ((1 << n) - 1), n)
            eobrun = 0
        for b in pending:
            out.put(b, 1)
        pending = []

    for m, k, c in blocks:
        blk = [int(v) for v in coefs[m, k]]
        code = codes.get(c)
        if Ss == 0 and Ah == 0:
            v = blk[0] >> Al                                 # the point transform of DC is an arithmetic shift (G.1.2.1)
            diff, pred[c] = v - pred[c], v
            n = abs(diff).bit_length()
            out.put(*code[n])
            out.put(diff if diff >= 0 else diff + (1 << n) - 1, n)
        elif Ss == 0:
            out.put((blk[0] >> Al) & 1, 1)
        elif Ah == 0:
            run = 0
            for z in range(Ss, Se + 1):
                t = abs(blk[z]) >> Al                        # AC: division towards zero (G.1.2.2)
                if t == 0:
                    run += 1
                    continue
                flush_eobrun(code)
                while run > 15:
                    out.put(*code[0xF0])
                    run -= 16
                n = t.bit_length()
                out.put(*code[run << 4 | n])
                out.put(t if blk[z] > 0 else (~t) & ((1 << n) - 1), n)
                run = 0
            if run:
                eobrun += 1
                if eobrun == 0x7FFF:
                    flush_eobrun(code)
        else:
            mags = [abs(v) >> Al for v in blk]
            last_new = max([z for z in range(Ss, Se + 1) if mags[z] == 1], default=-1)
            run, corr = 0, []
            for z in range(Ss, Se + 1):
                if mags[z] == 0:
                    run += 1
                    continue
                while run > 15 and z <= last_new:
                    flush_eobrun(code)
                    out.put(*code[0xF0])
                    run -= 16
                    for b in corr:
                        out.put(b, 1)
                    corr = []
                if mags[z] > 1:                              # a nonzero history: its next bit waits for the symbol that passes it
                    corr.append(mags[z] & 1)
                    continue
                flush_eobrun(code)
                out.put(*code[run << 4 | 1])
                out.put(1 if blk[z] > 0 else 0, 1)
                for b in corr:
                    out.put(b, 1)
                run, corr = 0, []
            if run or corr:
                eobrun += 1
                pending += corr
                if eobrun == 0x7FFF or len(pending) > 900:
                    flush_eobrun(code)
    if Ss:
        flush_eobrun(codes[blocks[0][2]])
    return out.bytes()


def _seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body


def write_progressive(coefs, quant, H, W, layout, script):
    """coefficients (n_mcu, bpm, 64) zig-zag, quant (3, 64) natural per component -> a progressive file under `script`: a list of dicts
    comps (component indices), Ss, Se, Ah, Al, and optionally tables ((td, ta) per component; default (0, 0) for component 0, (1, 1)
    for the others), dht ({(class, destination): a key of TABLES}, written in front of this scan; the first scan's default defines
    destinations 0 and 1 of both classes) and ri (the DRI in force from this scan on)."""
    nc, hs, vs = layout
    coefs = np.asarray(coefs)
    out = [b"\xFF\xD8", _seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")]
    for tq in range(nc):
        out.append(_seg(0xDB, bytes([tq]) + bytes(int(v) for v in np.asarray(quant)[tq][R.ZIGZAG])))
    factors = [(hs, vs), (1, 1), (1, 1)][:nc]
    out.append(_seg(0xC2, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([nc]) +
                    b"".join(bytes([i + 1, h << 4 | v, i]) for i, (h, v) in enumerate(factors))))
    huff, ri = {}, 0
    for n, sc in enumerate(script):
        dht = sc.get("dht", {(0, 0): "dcA", (0, 1): "dcB", (1, 0): "acA", (1, 1): "acB"} if n == 0 else {})
        for (tc, th), name in dht.items():
            huff[(tc, th)] = TABLES[name]
            out.append(_seg(0xC4, bytes([tc << 4 | th]) + bytes(TABLES[name][0]) + TABLES[name][1]))
        if sc.get("ri", ri) != ri:
            ri = sc["ri"]
            out.append(_seg(0xDD, ri.to_bytes(2, "big")))
        tables = sc.get("tables", tuple((0, 0) if c == 0 else (1, 1) for c in sc["comps"]))
        ah_al = sc["Ah"] << 4 | sc["Al"]
        out.append(_seg(0xDA, bytes([len(sc["comps"])]) + b"".join(bytes([c + 1, td << 4 | ta]) for c, (td, ta) in zip(sc["comps"], tables)) +
                        bytes([sc["Ss"], sc["Se"], ah_al])))
        codes = {c: _codes(huff[(0, td) if sc["Ss"] == 0 else (1, ta)]) for c, (td, ta) in zip(sc["comps"], tables)}
        blocks = scan_blocks(H, W, layout, sc["comps"])
        per_unit = L.bpm(layout) if len(sc["comps"]) == nc else 1
        units = len(blocks) // per_unit
        step = ri or units
        for i, u0 in enumerate(range(0, units, step)):
            if i:
                out.append(bytes([0xFF, 0xD0 + (i - 1) % 8]))
            out.append(_encode_interval(blocks[u0 * per_unit:min(u0 + step, units) * per_unit], coefs, sc, codes))
    out.append(b"\xFF\xD9")
    return b"".join(out)


def _scan(comps, Ss, Se, Ah, Al, **kw):
    return dict(comps=tuple(comps), Ss=Ss, Se=Se, Ah=Ah, Al=Al, **kw)


def scripts(nc, restart=True):
    """the scripts Pillow never writes, by name, for nc components; restart=False: the "restart" script without its intervals"""
    each = list(range(nc))
    both = tuple(each)
    spectral = [_scan(both, 0, 0, 0, 0)] + [s for c in each for s in (_scan([c], 1, 5, 0, 0), _scan([c], 6, 63, 0, 0))]
    out = {
        "spectral selection only": spectral,
        "one DC scan per component": [_scan([c], 0, 0, 0, 0) for c in each] + [_scan([c], 1, 63, 0, 0) for c in each],
        "three approximation steps": [_scan(both, 0, 0, 0, 2), _scan(both, 0, 0, 2, 1)] + [_scan([c], 1, 63, 0, 2) for c in each] +
                                     [_scan([c], 1, 63, 2, 1) for c in each] + [_scan(both, 0, 0, 1, 0)] + [_scan([c], 1, 63, 1, 0) for c in each],
    }
    # Cb and Cr on different DC and AC destinations, all four destinations of both classes defined and read, one redefined between scans
    dht = {(0, 0): "dcA", (0, 1): "dcB", (0, 2): "dcC", (0, 3): "dcB", (1, 0): "acA", (1, 1): "acB", (1, 2): "acC", (1, 3): "acB"}
    tabs = [(3, 0), (1, 1), (2, 2)]
    out["four destinations"] = ([_scan(both, 0, 0, 0, 1, tables=tuple(tabs[:nc]), dht=dht), _scan([0], 1, 5, 0, 0, tables=((3, 0),))] +
                                [_scan([c], 1, 63, 0, 0, tables=(tabs[c],)) for c in each[1:]] +
                                [_scan([0], 6, 20, 0, 0, tables=((3, 3),)), _scan([0], 21, 63, 0, 0, tables=((3, 1),), dht={(1, 1): "acC", (0, 0): "dcC"}),
                                 _scan([0], 0, 0, 1, 0, tables=((0, 0),))] + [_scan([c], 0, 0, 1, 0, tables=(tabs[c],)) for c in each[1:]])
    # intervals of 3 units, which do not divide the unit counts, for some scans and none for others
    ris = [3, 0, 3, 3, 0, 3, 0]
    out["restart"] = [dict(s, ri=(ris[i % len(ris)] if restart else 0)) for i, s in enumerate(spectral)]
    return out
