"""What the GIF reader's tests measure against, in numpy and plain Python, independent of emote_hack_amd: a general LZW decoder for code
sizes 2 .. 8 that takes what Pillow takes (no leading Clear, a full table without a Clear, several Clears, KwKwK, no End of Information,
data behind the last pixel) and names what it does not with the statuses of include/emo_hip.h; an LZW encoder with switches that builds
such streams; a container builder; and the six composition rules of emo_gif_compose, interlace included.  tests/test_gif_decode_host.py
holds this reference against Pillow, file by file and byte for byte; the GPU tests then hold the kernels against it."""
import struct

import numpy as np

OK, BAD_CODE, PAST_END, SHORT, BAD_INDEX, BAD_FRAME = 0, 1, 2, 3, 4, 8           # EMO_GIF_*
TABLE_MAX = 4096


# ------------------------------------------------------------------------------------------------------------------------------ LZW
def lzw_decode(data, code_size, n_pixels):
    """image data (sub-blocks joined) -> (indices as bytes: what was produced, status).  Entries as byte strings, chains and all: the
    textbook decoder, nothing of the kernel's (start, length) trick."""
    clear, eoi = 1 << code_size, (1 << code_size) + 1
    table = [bytes([i]) for i in range(clear)] + [b"", b""]
    width, prev, out = code_size + 1, None, bytearray()
    acc = nbits = pos = 0
    while len(out) < n_pixels:
        while nbits < width:
            if pos >= len(data):
                return bytes(out), PAST_END
            acc |= data[pos] << nbits
            nbits += 8
            pos += 1
        code = acc & ((1 << width) - 1)
        acc >>= width
        nbits -= width
        if code == clear:
            del table[clear + 2:]
            width, prev = code_size + 1, None
            continue
        if code == eoi:
            return bytes(out), SHORT
        if prev is None:
            if code > clear:
                return bytes(out), BAD_CODE
            entry = table[code]
        else:
            if code < len(table):
                entry = table[code]
            elif code == len(table) and len(table) < TABLE_MAX:
                entry = prev + prev[:1]
            else:
                return bytes(out), BAD_CODE
            if len(table) < TABLE_MAX:
                table.append(prev + entry[:1])
                if len(table) == 1 << width and width < 12:
                    width += 1
        out += entry[:n_pixels - len(out)]
        prev = entry
    return bytes(out), OK


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, width):
        self.acc |= code << self.n
        self.n += width
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def lzw_encode(indices, code_size=8, leading_clear=True, clear_when_full=True, eoi=True, double_clear=False, record=None):
    """palette indices (any shape, values below 1 << code_size) -> image data.  The encoder tracks the DECODER's table to write every
    code at the width the decoder holds.  leading_clear=False starts without a Clear; clear_when_full=False never clears - once the
    table is full the encoder goes on with the frozen table at 12 bits (the deferred clear); eoi=False leaves End of Information out;
    double_clear writes two Clears where one is due.  record (a dict) takes `codes`, `max_len`, `kwkwk` and `full` for the host test."""
    clear, end = 1 << code_size, (1 << code_size) + 1
    w = BitWriter()
    state = dict(width=code_size + 1, next=clear + 2, prev=False)
    stats = dict(codes=0, max_len=0, kwkwk=0, full=False)

    def emit(code):
        w.put(code, state["width"])
        stats["codes"] += 1
        if code == clear:
            state.update(width=code_size + 1, next=clear + 2, prev=False)
            return
        if state["prev"]:
            if code == state["next"] and state["next"] < TABLE_MAX:
                stats["kwkwk"] += 1
            if state["next"] < TABLE_MAX:
                state["next"] += 1
                if state["next"] == 1 << state["width"] and state["width"] < 12:
                    state["width"] += 1
        state["prev"] = True

    def do_clear():
        emit(clear)
        if double_clear:
            emit(clear)

    if leading_clear:
        do_clear()
    table, free, cur, cur_len = {}, clear + 2, None, 0
    for k in np.asarray(indices).reshape(-1).tolist():
        if cur is None:
            cur, cur_len = k, 1
        elif (cur, k) in table:
            cur, cur_len = table[cur, k], cur_len + 1
        else:
            emit(cur)
            stats["max_len"] = max(stats["max_len"], cur_len)
            if free < TABLE_MAX:
                table[cur, k] = free
                free += 1
            else:
                stats["full"] = True
                if clear_when_full:
                    do_clear()
                    table, free = {}, clear + 2
            cur, cur_len = k, 1
    if cur is not None:
        emit(cur)
        stats["max_len"] = max(stats["max_len"], cur_len)
    if eoi:
        emit(end)
    if record is not None:
        record.update(stats)
    return w.done()


def pack_codes(codes):
    """[(code, width)] -> bytes: a stream written by hand, for the codes no encoder writes"""
    w = BitWriter()
    for code, width in codes:
        w.put(code, width)
    return w.done()


# ------------------------------------------------------------------------------------------------------------------------------ container
def sub_blocks(stream, size=255):
    out = bytearray()
    for at in range(0, len(stream), size):
        part = stream[at:at + size]
        out += bytes([len(part)]) + part
    return bytes(out) + b"\x00"


def interlace_rows(h):
    """the canvas rows of a frame of h rows in the order an interlaced stream holds them (GIF89a Appendix E)"""
    return [*range(0, h, 8), *range(4, h, 8), *range(2, h, 4), *range(1, h, 2)]


def frame(indices, left=0, top=0, table=None, transparent=None, disposal=None, delay=None, interlace=False, code_size=None, data=None,
          control=None, **lzw):
    """one frame for build(): indices (h, w) uint8; table (k, 3) uint8 local table or None; a graphic control extension is written when
    any of transparent, disposal, delay is given (control=False: never, True: always).  data= overrides the image data."""
    indices = np.asarray(indices, np.uint8)
    if control is None:
        control = transparent is not None or disposal is not None or delay is not None
    return dict(indices=indices, left=left, top=top, table=None if table is None else np.asarray(table, np.uint8), transparent=transparent,
                disposal=disposal or 0, delay=delay or 0, interlace=interlace, code_size=code_size, data=data, control=control, lzw=lzw)


def table_bits(k):
    bits = max(1, int(np.ceil(np.log2(max(k, 2)))))
    assert 2 ** bits == k, f"a GIF colour table holds 2, 4, ... 256 entries, not {k}"
    return bits - 1


def build(width, height, frames, global_table=None, background=0, loop=None, version=b"GIF89a", trailer=True, comment=None):
    """-> the file's bytes.  frames: frame() dicts."""
    out = [version]
    flags = 0 if global_table is None else 0x80 | table_bits(len(global_table)) | 0x70
    out.append(struct.pack("<HHBBB", width, height, flags, background, 0))
    if global_table is not None:
        out.append(np.asarray(global_table, np.uint8).tobytes())
    if loop is not None:
        out.append(b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00")
    if comment is not None:
        out.append(b"\x21\xFE" + sub_blocks(comment))
    for f in frames:
        h, w = f["indices"].shape
        if f["control"]:
            packed = (f["disposal"] << 2) | (1 if f["transparent"] is not None else 0)
            out.append(b"\x21\xF9\x04" + struct.pack("<BHB", packed, f["delay"], f["transparent"] or 0) + b"\x00")
        packed = (0x40 if f["interlace"] else 0) | (0 if f["table"] is None else 0x80 | table_bits(len(f["table"])))
        out.append(b"\x2C" + struct.pack("<HHHHB", f["left"], f["top"], w, h, packed))
        if f["table"] is not None:
            out.append(f["table"].tobytes())
        entries = len(f["table"]) if f["table"] is not None else len(global_table) if global_table is not None else 256
        cs = f["code_size"] or max(2, int(np.ceil(np.log2(entries))))
        stream = f["indices"][interlace_rows(h)] if f["interlace"] else f["indices"]
        data = f["data"] if f["data"] is not None else lzw_encode(stream, cs, **f["lzw"])
        out.append(bytes([cs]) + sub_blocks(data))
    if trailer:
        out.append(b"\x3B")
    return b"".join(out)


# ------------------------------------------------------------------------------------------------------------------------------ composition
def stream_row(y, h):
    """the row of an interlaced frame's stream that its canvas row y reads: the closed form emo_gif_compose uses"""
    a, b, c = -(-h // 8), -(-max(h - 4, 0) // 8), -(-max(h - 2, 0) // 4)
    if y % 8 == 0:
        return y // 8
    if y % 8 == 4:
        return a + (y - 4) // 8
    if y % 4 == 2:
        return a + b + (y - 2) // 4
    return a + b + c + (y - 1) // 2


def compose(width, height, frames, global_table=None, background=0):
    """the six rules -> uint8 (n, height, width, 3): the canvas after every frame.  frames: frame() dicts, whose `indices` are in CANVAS
    order (build() interlaces them)."""
    bg = background if global_table is not None else 0
    canvas = np.zeros((height, width, 3), np.uint8)
    out, sticky, pending = [], 0, None
    for k, f in enumerate(frames):
        pal = np.zeros((256, 3), np.uint8)
        src = f["table"] if f["table"] is not None else global_table
        pal[:len(src)] = src
        t = f["transparent"] if f["control"] else None
        h, w = f["indices"].shape
        y0, x0 = f["top"], f["left"]
        if pending is not None:
            pending(canvas)
        if k == 0:
            canvas[:] = pal[t] if t is not None else pal[0]                      # rule 2
        before = canvas[y0:y0 + h, x0:x0 + w].copy()
        colours = pal[f["indices"]]
        if k == 0 or t is None:
            canvas[y0:y0 + h, x0:x0 + w] = colours
        else:                                                                    # rule 5
            drawn = f["indices"] != t
            canvas[y0:y0 + h, x0:x0 + w][drawn] = colours[drawn]
        out.append(canvas.copy())
        if f["control"] and f["disposal"]:
            sticky = min(f["disposal"], 3)                                       # rule 3
        pending = None
        if sticky == 2:                                                          # rule 4
            fill = pal[t] if t is not None else pal[bg if bg < len(src) else 0]
            pending = lambda c, y0=y0, x0=x0, h=h, w=w, fill=fill: c[y0:y0 + h, x0:x0 + w].__setitem__(slice(None), fill)
        elif sticky == 3:
            if k > 0:
                pending = lambda c, y0=y0, x0=x0, h=h, w=w, before=before: c[y0:y0 + h, x0:x0 + w].__setitem__(slice(None), before)
            elif t is not None:
                pending = lambda c, y0=y0, x0=x0, h=h, w=w, fill=pal[t].copy(): c[y0:y0 + h, x0:x0 + w].__setitem__(slice(None), fill)
    return np.stack(out)


def compose_descriptors(indices, desc, tables, height, width):
    """emo_gif_compose restated: indices - per frame its colour indices in STREAM order -, desc int (n, 11) as the entry takes them,
    tables uint8 (n_tables, 256, 3) -> (uint8 (n, height, width, 3): the canvas after every frame, status per frame)"""
    canvas = np.zeros((height, width, 3), np.uint8)
    saved = canvas.copy()
    out, status, prev = [], [], None
    for k, d in enumerate(np.asarray(desc).tolist()):
        left, top, w, h, t, disposal, fill, lace, row, entries, _ = d
        pal = tables[row]
        if k == 0:
            canvas[:] = pal[t if t >= 0 else 0]
        if prev is not None and prev[0] >= 2:
            _, x0, y0, pw, ph, colour = prev
            canvas[y0:y0 + ph, x0:x0 + pw] = colour if prev[0] == 2 else saved[y0:y0 + ph, x0:x0 + pw]
        saved = canvas.copy()
        idx = np.frombuffer(bytes(indices[k]), np.uint8).reshape(h, w)
        if lace:
            idx = idx[[stream_row(y, h) for y in range(h)]]
        drawn = np.ones((h, w), bool) if k == 0 else idx != t
        canvas[top:top + h, left:left + w][drawn] = pal[idx][drawn]
        status.append(BAD_INDEX if (idx[drawn] >= entries).any() else OK)
        out.append(canvas.copy())
        prev = (disposal, left, top, w, h, pal[fill].copy())
    return np.stack(out), status


def pillow_frames(data):
    """every frame of the file as Pillow gives it: seek(k), convert("RGB")"""
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    out = []
    for k in range(getattr(im, "n_frames", 1)):
        im.seek(k)
        out.append(np.asarray(im.convert("RGB")).copy())
    return np.stack(out)
