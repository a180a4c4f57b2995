"""The inputs the PNG reader's host and GPU tests share: Pillow files, zlib streams with flushes in the middle, hand-built deflate
streams for what zlib's own matcher never writes, and streams damaged in one named way each.  The host tests check every one of them
against zlib and assert from the reference's record that it holds the case it is here for; the GPU tests run them."""
import functools
import io
import zlib

import numpy as np
from PIL import Image

from tests import png_decode_ref as D

FAR = 130 * 258           # grey 257 x 130: the smallest frame whose bytes pass offset 32768 with room for a match of 258 behind it
SMALL = 100               # bytes of the frames the damaged streams stand in


def raw_inflate(stream):
    """zlib's answer to a raw deflate stream; zlib.error where it has one"""
    d = zlib.decompressobj(-15)
    out = d.decompress(stream)
    if not d.eof:
        raise zlib.error("incomplete or truncated stream")
    return out


def shape_of(nbytes):
    """(H, W, C) of a frame with that many filtered bytes: one grey row"""
    return 1, nbytes - 1, 1


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def pillow_file(array, **options):
    b = io.BytesIO()
    Image.fromarray(array).save(b, "PNG", **options)
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def pillow_images():
    """name -> (H, W, 3) arrays whose Pillow files hold stored, fixed and dynamic blocks"""
    ramp = np.add.outer(np.arange(64), np.arange(64))[..., None] * np.array([1, 2, 3])
    out = {"noise64": noise((64, 64, 3), 1), "noise160": noise((160, 160, 3), 2), "tiny": noise((2, 2, 3), 3),
           "flat": np.full((64, 64, 3), 77, np.uint8), "gradient": (ramp % 256).astype(np.uint8)}
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pillow_files():
    return {k: pillow_file(a) for k, a in pillow_images().items()}


def text(n, seed):
    """compressible bytes: words of a small vocabulary"""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, rng.integers(2, 9), dtype=np.uint8)) for _ in range(40)]
    out = b" ".join(words[i] for i in rng.integers(0, 40, n))
    return out[:n]


@functools.lru_cache(maxsize=None)
def zlib_streams():
    """name -> (raw deflate stream, the bytes it holds): levels 1 and 9, sync and full flushes in the middle (empty stored blocks that
    start at whatever bit the block before ended on)"""
    out = {}
    data = text(3001, 5)
    for level in (1, 9):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        out[f"level{level}"] = (c.compress(data) + c.flush(), data)
    for level, cuts in ((6, (700, 1501, 2222)), (1, (1, 2, 3, 50, 51, 1000, 2999))):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        parts, at = [], 0
        for k, cut in enumerate(cuts):
            parts.append(c.compress(data[at:cut]) + c.flush(zlib.Z_FULL_FLUSH if k % 2 else zlib.Z_SYNC_FLUSH))
            at = cut
        out[f"flushes{level}"] = (b"".join(parts) + c.compress(data[at:]) + c.flush(), data)
    return out


@functools.lru_cache(maxsize=None)
def hand_streams():
    """name -> (raw deflate stream, the bytes it holds)"""
    out = {}
    # every length and distance at which the 64-lane copy changes its step count or overlaps itself, both pairings
    w, tokens = D.DeflateWriter(), [bytes(noise(70, 7))]
    w.fixed(final=True)
    w.literal(tokens[0])
    lengths, distances = (3, 64, 65, 128, 129, 258), (1, 2, 3, 63, 64, 65)
    for l, d in list(zip(lengths, distances)) + list(zip(lengths, reversed(distances))):
        w.match(l, d)
        tokens.append((l, d))
    w.end()
    out["lengths"] = (w.done(), D.apply_tokens(tokens))
    # a distance equal to the bytes produced so far, at 1 and at 8
    w = D.DeflateWriter()
    w.fixed(final=True)
    w.literal(b"a"); w.match(5, 1); w.literal(b"bc"); w.match(4, 8)
    w.end()
    out["whole_history"] = (w.done(), D.apply_tokens([b"a", (5, 1), b"bc", (4, 8)]))
    # FAR bytes: a match over the whole history whose destination crosses offset 32768, then a stored block from an odd bit on
    head, tail = bytes(noise(32700, 8)), bytes(noise(FAR - 32700 - 258, 9))
    w = D.DeflateWriter()
    w.stored(head)
    w.fixed()
    w.match(258, 32700)
    w.end()
    w.stored(tail, final=True)
    out["far_dest"] = (w.done(), D.apply_tokens([head, (258, 32700), tail]))
    # FAR bytes: a stored block across offset 32768, distance 32768, a match whose source crosses the offset
    head = bytes(noise(33000, 10))
    tail = bytes(noise(FAR - 33000 - 258 - 200, 11))
    w = D.DeflateWriter()
    w.stored(head)
    w.fixed(final=True)
    w.match(258, 32768); w.match(200, 600); w.literal(tail)
    w.end()
    out["far_source"] = (w.done(), D.apply_tokens([head, (258, 32768), (200, 600), tail]))
    # codes of 1 .. 15 bits, and a block without distance codes
    lit = [0] * 257
    for s in range(15):
        lit[s] = s + 1
    lit[256] = 15
    data = bytes(list(range(15)) * 3 + [14, 14, 0, 13])
    w = D.DeflateWriter()
    w.dynamic(lit, [0], final=True)
    w.literal(data)
    w.end()
    out["code15"] = (w.done(), data)
    # a distance set of one single code
    lit = [0] * 286
    lit[97] = lit[256] = lit[257] = lit[285] = 2
    w = D.DeflateWriter()
    w.dynamic(lit, [1], final=True)
    w.literal(b"a"); w.match(3, 1); w.match(258, 1)
    w.end()
    out["one_distance"] = (w.done(), b"a" * 262)
    # a repeat of the code lengths that runs from the literal / length lengths into the distance lengths
    lit = [0] * 257
    lit[97] = lit[98] = lit[255] = lit[256] = 2
    runs = [(18, 97 - 11), (2, 0), (2, 0), (18, 138 - 11), (18, 18 - 11), (2, 0), (16, 0), (2, 0), (2, 0)]
    w = D.DeflateWriter()
    w.dynamic(lit, [2, 2, 2, 2], final=True, runs=runs)
    w.literal(b"abab\xffa")
    w.end()
    out["repeat_crosses"] = (w.done(), b"abab\xffa")
    return out


def healthy(n=SMALL):
    """(raw deflate stream, its n bytes): a dynamic block of zlib's"""
    data = text(n, 12)
    c = zlib.compressobj(9, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush(), data


@functools.lru_cache(maxsize=None)
def damaged_streams():
    """name -> (raw deflate stream, the status it must end with in a frame of SMALL bytes); each damaged in one way"""
    out = {}
    out["block_type_3"] = (bytes([0b111, 0, 0, 0]), D.BAD_BLOCK)
    w = D.DeflateWriter()
    w.stored(b"hello", final=True, nlen=(5 ^ 0xFFFF) ^ 0x0100)
    out["flipped_nlen"] = (w.done(), D.BAD_STORED)

    def header(lit_codes, dist=(0,), **kw):
        lit = [0] * 257
        for s, l in lit_codes.items():
            lit[s] = l
        w = D.DeflateWriter()
        w.dynamic(lit, list(dist), final=True, **kw)
        w.put(0, 32)
        return w.done()
    out["over_subscribed"] = (header({97: 1, 98: 1, 256: 1}), D.BAD_LENGTHS)
    out["incomplete"] = (header({97: 2, 256: 2}), D.BAD_LENGTHS)
    out["over_subscribed_distances"] = (header({97: 1, 256: 1}, dist=(1, 1, 1)), D.BAD_LENGTHS)
    out["no_end_of_block"] = (header({97: 1, 98: 1}), D.BAD_LENGTHS)
    out["repeat_first"] = (header({97: 1, 256: 1}, runs=[(16, 0), (18, 127)]), D.BAD_LENGTHS)
    out["repeat_past_end"] = (header({97: 1, 256: 1}, runs=[(18, 127), (18, 127)]), D.BAD_LENGTHS)
    out["incomplete_code_length_code"] = (header({97: 1, 256: 1}, cl=[4] * 12 + [0] + [5] * 6), D.BAD_LENGTHS)
    w = D.DeflateWriter()
    w.fixed(final=True)
    w.literal(b"ab"); w.symbol(286); w.put(0, 32)
    out["symbol_286"] = (w.done(), D.BAD_SYMBOL)
    w = D.DeflateWriter()
    w.fixed(final=True)
    w.literal(b"ab"); w.symbol(257); w.distance_symbol(30); w.put(0, 32)
    out["distance_symbol_30"] = (w.done(), D.BAD_SYMBOL)
    lit = [0] * 286
    lit[97] = lit[256] = lit[257] = lit[285] = 2
    w = D.DeflateWriter()
    w.dynamic(lit, [1], final=True)
    w.literal(b"a"); w.symbol(257); w.put(1, 1); w.put(0, 32)                    # the one distance code is the bit 0
    out["bits_of_no_code"] = (w.done(), D.BAD_SYMBOL)
    w = D.DeflateWriter()
    w.fixed(final=True)
    w.literal(b"a"); w.match(3, 2); w.end()
    out["distance_too_far"] = (w.done(), D.BAD_DISTANCE)
    w = D.DeflateWriter()
    w.fixed(final=True)
    w.literal(b"a"); w.put(0b1001, 4)                                            # the first four bits of the eight of another `a`
    out["cut_in_a_code"] = (w.done(), D.PAST_END)
    out["cut_in_half"] = (healthy()[0][:len(healthy()[0]) // 2], D.PAST_END)
    out["empty"] = (b"", D.PAST_END)
    out["one_byte_more"] = (healthy(SMALL + 1)[0], D.OVERFLOW)
    out["one_byte_less"] = (healthy(SMALL - 1)[0], D.SHORT)
    return out


def all_streams():
    """name -> (raw deflate stream, its bytes) of every healthy stream the GPU tests inflate"""
    from emote_hack_amd import video_io as V
    out = {}
    for k, f in pillow_files().items():
        p = V.parse_png(f)
        out[f"pillow_{k}"] = (p.still, raw_inflate(p.still))
    out.update(zlib_streams())
    out.update(hand_streams())
    out["healthy"] = healthy()
    return out
