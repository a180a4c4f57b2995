"""What the PNG reader's tests measure against, in plain Python and numpy, written from RFC 1951 and PNG section 9 and independent of the
kernels: a serial inflate in the manner of puff (canonical codes walked bit by bit, one count per length) that returns the bytes, the
status under the names of include/emo_hip.h, and a record of what it met on the way - so a test asserts that its input really holds
the case it claims; an LSB-first bit writer for hand-built streams (stored blocks, fixed codes, dynamic headers spelt out run by run);
and the five filters undone row by row."""
import numpy as np

from tests.png_ref import DIST_BASE, DIST_EXTRA, LENGTH_BASE, LENGTH_EXTRA, paeth

OK, BAD_BLOCK, BAD_STORED, BAD_LENGTHS, BAD_SYMBOL, BAD_DISTANCE, PAST_END, OVERFLOW, SHORT, BAD_FILTER = range(10)      # EMO_PNG_*
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
WINDOW = 32768


class _End(Exception):
    def __init__(self, status):
        self.status = status


class _Bits:
    def __init__(self, data):
        self.data, self.pos = bytes(data), 0                                     # pos in bits

    def take(self, n):
        v = 0
        for k in range(n):
            if self.pos >= 8 * len(self.data):
                raise _End(PAST_END)
            v |= (self.data[self.pos >> 3] >> (self.pos & 7) & 1) << k
            self.pos += 1
        return v


def _counts(lengths):
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    return count


def code_space_left(lengths):
    """what a set of code lengths leaves of the code space: negative over-subscribed, 0 complete, positive incomplete"""
    count, left = _counts(lengths), 1
    for l in range(1, 16):
        left = left * 2 - count[l]
        if left < 0:
            return left
    return left


def set_is_bad(lengths, code_length_code=False):
    """zlib's inflate_table: over-subscribed is bad; incomplete is bad unless the set is one code of one bit or (not for the code-length
    code) no code at all"""
    left, longest = code_space_left(lengths), max(lengths, default=0)
    if left < 0:
        return True
    if code_length_code:
        return left != 0
    return left > 0 and longest > 1


def _decode(bits, lengths, record=None):
    """puff's decode: -> the symbol, or None when 15 bits begin no code"""
    count = _counts(lengths)
    symbols = [s for l in range(1, 16) for s, sl in enumerate(lengths) if sl == l]
    code = first = index = 0
    start = bits.pos
    for l in range(1, 16):
        if bits.pos >= 8 * len(bits.data):
            raise _End(PAST_END)
        code |= bits.take(1)
        if code - count[l] < first:
            if record is not None:
                record["longest_code"] = max(record["longest_code"], l)
            return symbols[index + code - first]
        index += count[l]
        first = (first + count[l]) << 1
        code <<= 1
    bits.pos = start
    return None


def new_record():
    return {"blocks": [], "longest_code": 0, "lengths": set(), "distances": set(), "whole_history": False, "source_crosses": False,
            "dest_crosses": False, "stored_crosses": False, "stored_bit_positions": set(), "empty_stored": 0, "one_code_distance_set": False,
            "no_distance_codes": False, "repeat_crosses": False}


def inflate(data, cap=None):
    """A raw deflate stream -> (the bytes produced, the status, the record).  cap: the bytes the frame holds (H * R): a token that would
    pass it ends the stream with OVERFLOW and writes nothing, a final block that ends before it gives SHORT; None: no limit"""
    bits, out, rec = _Bits(data), bytearray(), new_record()
    try:
        while True:
            last, kind = bits.take(1), bits.take(2)
            rec["blocks"].append(kind)
            if kind == 3:
                raise _End(BAD_BLOCK)
            if kind == 0:
                rec["stored_bit_positions"].add(bits.pos & 7)
                bits.pos = (bits.pos + 7) & ~7
                n, inv = bits.take(16), bits.take(16)
                if n ^ inv != 0xFFFF:
                    raise _End(BAD_STORED)
                at = bits.pos >> 3
                if at + n > len(bits.data):
                    raise _End(PAST_END)
                if cap is not None and len(out) + n > cap:
                    raise _End(OVERFLOW)
                rec["empty_stored"] += n == 0
                rec["stored_crosses"] |= len(out) < WINDOW < len(out) + n
                out += bits.data[at:at + n]
                bits.pos += 8 * n
            else:
                if kind == 1:
                    lit, dist = FIXED_LIT, FIXED_DIST
                else:
                    lit, dist = _dynamic(bits, rec)
                while True:
                    s = _decode(bits, lit, rec)
                    if s is None or s > 285:
                        raise _End(PAST_END if s is None and 8 * len(bits.data) - bits.pos < 15 else BAD_SYMBOL)
                    if s == 256:
                        break
                    if s < 256:
                        if cap is not None and len(out) >= cap:
                            raise _End(OVERFLOW)
                        out.append(s)
                        continue
                    length = LENGTH_BASE[s - 257] + bits.take(LENGTH_EXTRA[s - 257])
                    d = _decode(bits, dist, rec)
                    if d is None or d > 29:
                        raise _End(PAST_END if d is None and 8 * len(bits.data) - bits.pos < 15 else BAD_SYMBOL)
                    distance = DIST_BASE[d] + bits.take(DIST_EXTRA[d])
                    if distance > len(out):
                        raise _End(BAD_DISTANCE)
                    if cap is not None and len(out) + length > cap:
                        raise _End(OVERFLOW)
                    pos = len(out)
                    rec["lengths"].add(length)
                    rec["distances"].add(distance)
                    rec["whole_history"] |= distance == pos
                    rec["source_crosses"] |= pos - distance < WINDOW < pos - distance + min(length, distance)
                    rec["dest_crosses"] |= pos < WINDOW < pos + length
                    for _ in range(length):
                        out.append(out[-distance])
            if last:
                break
    except _End as e:
        return bytes(out), e.status, rec
    return bytes(out), SHORT if cap is not None and len(out) < cap else OK, rec


def _dynamic(bits, rec):
    hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
    if hlit > 286 or hdist > 30:
        raise _End(BAD_LENGTHS)
    cl = [0] * 19
    for k in range(hclen):
        cl[CL_ORDER[k]] = bits.take(3)
    if set_is_bad(cl, code_length_code=True):
        raise _End(BAD_LENGTHS)
    lengths = []
    while len(lengths) < hlit + hdist:
        s = _decode(bits, cl)
        if s is None:
            raise _End(PAST_END if 8 * len(bits.data) - bits.pos < 15 else BAD_LENGTHS)
        if s < 16:
            lengths.append(s)
            continue
        if s == 16:
            if not lengths:
                raise _End(BAD_LENGTHS)
            value, rep = lengths[-1], 3 + bits.take(2)
        elif s == 17:
            value, rep = 0, 3 + bits.take(3)
        else:
            value, rep = 0, 11 + bits.take(7)
        if len(lengths) + rep > hlit + hdist:
            raise _End(BAD_LENGTHS)
        rec["repeat_crosses"] |= len(lengths) < hlit < len(lengths) + rep
        lengths += [value] * rep
    lit, dist = lengths[:hlit], lengths[hlit:]
    if lit[256] == 0 or set_is_bad(lit) or set_is_bad(dist):
        raise _End(BAD_LENGTHS)
    rec["one_code_distance_set"] |= sum(dist) == 1                              # one code, of one bit
    rec["no_distance_codes"] |= not any(dist)
    return lit, dist


# ------------------------------------------------------------------------------------------------------------------------------ writer
def canonical(lengths):
    """RFC 1951 3.2.2: lengths -> codes (read most significant bit first)"""
    count = _counts(lengths)
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    codes = []
    for l in lengths:
        codes.append(nxt[l])
        nxt[l] += 1 if l else 0
    return codes


class DeflateWriter:
    """Hand-built deflate streams, least significant bit first.  stored(); fixed() or dynamic() open a block whose literal(), match(),
    symbol() and end() then use its codes.  Nothing is checked: a test may write what no encoder would."""
    DEFAULT_CL = [4] * 13 + [5] * 6                                               # a complete code over all 19 code-length symbols

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0
        self.lit = self.dist = None

    def put(self, value, width):
        self.acc |= (value & ((1 << width) - 1)) << self.n
        self.n += width
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def put_code(self, code, length):
        for k in range(length - 1, -1, -1):
            self.put(code >> k & 1, 1)

    def done(self):
        return bytes(self.out) + (bytes([self.acc & 255]) if self.n else b"")

    def stored(self, data, final=False, nlen=None):
        self.put(int(final), 1)
        self.put(0, 2)
        if self.n:
            self.put(0, 8 - self.n)
        self.put(len(data), 16)
        self.put(len(data) ^ 0xFFFF if nlen is None else nlen, 16)
        self.out += bytes(data)

    def _codes(self, lit, dist):
        self.lit, self.dist = (list(lit), canonical(lit)), (list(dist), canonical(dist))

    def fixed(self, final=False):
        self.put(int(final), 1)
        self.put(1, 2)
        self._codes(FIXED_LIT, FIXED_DIST)

    def dynamic(self, lit, dist, final=False, runs=None, cl=None, hlit=None, hdist=None):
        """lit, dist: the code lengths (hlit, hdist default to their counts).  runs: the code-length symbols as [(symbol, extra value)];
        default one symbol per length, no repeats.  cl: the 19 lengths of the code-length code"""
        cl = list(self.DEFAULT_CL if cl is None else cl)
        runs = [(l, 0) for l in list(lit) + list(dist)] if runs is None else runs
        self.put(int(final), 1)
        self.put(2, 2)
        self.put((len(lit) if hlit is None else hlit) - 257, 5)
        self.put((len(dist) if hdist is None else hdist) - 1, 5)
        self.put(19 - 4, 4)
        for s in CL_ORDER:
            self.put(cl[s], 3)
        codes = canonical(cl)
        for s, x in runs:
            self.put_code(codes[s], cl[s])
            self.put(x, {16: 2, 17: 3, 18: 7}.get(s, 0))
        self._codes(lit, dist)

    def symbol(self, s):
        self.put_code(self.lit[1][s], self.lit[0][s])

    def literal(self, data):
        for b in bytes([data]) if isinstance(data, int) else bytes(data):
            self.symbol(b)

    def distance_symbol(self, d, extra=0):
        self.put_code(self.dist[1][d], self.dist[0][d])
        self.put(extra, DIST_EXTRA[d] if d < 30 else 0)

    def match(self, length, distance):
        k = 28 if length == 258 else max(i for i in range(28) if LENGTH_BASE[i] <= length)
        self.symbol(257 + k)
        self.put(length - LENGTH_BASE[k], LENGTH_EXTRA[k])
        d = max(i for i in range(30) if DIST_BASE[i] <= distance)
        self.distance_symbol(d, distance - DIST_BASE[d])

    def end(self):
        self.symbol(256)


def apply_tokens(tokens):
    """[bytes | (length, distance)] -> the bytes they stand for"""
    out = bytearray()
    for t in tokens:
        if isinstance(t, tuple):
            for _ in range(t[0]):
                out.append(out[-t[1]])
        else:
            out += t
    return bytes(out)


# ------------------------------------------------------------------------------------------------------------------------------ unfilter
def unfilter(filtered, C):
    """uint8 (n, H, 1 + W * C) -> uint8 (n, H, W, C) (PNG 9.2 - 9.4; a type above 4 raises ValueError)"""
    n, H, R = filtered.shape
    out = np.zeros((n, H, R - 1), np.uint8)
    for f in range(n):
        above = [0] * (R - 1)
        for y in range(H):
            t, x, row = int(filtered[f, y, 0]), filtered[f, y, 1:].tolist(), [0] * (R - 1)
            if t > 4:
                raise ValueError(f"filter type {t}")
            for j in range(R - 1):
                a = row[j - C] if j >= C else 0
                b = above[j]
                c = above[j - C] if j >= C else 0
                pred = (0, a, b, (a + b) >> 1, paeth(a, b, c) if t == 4 else 0)[t]
                row[j] = (x[j] + pred) & 255
            out[f, y] = above = row
    return out.reshape(n, H, (R - 1) // C, C)
