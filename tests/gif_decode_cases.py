"""The named cases of the GIF reader's tests: the smallest shapes that reach each path of emo_gif_lzw_decode and emo_gif_compose
(csrc/gif_in.hip).  tests/test_gif_decode_host.py asserts what each case claims (that the table fills, that every code is KwKwK, ...) and
holds the reference against Pillow on them; tests/test_gpu_gif_decode.py holds the kernels against the reference."""
import functools
import io

import numpy as np

from tests import gif_decode_ref as R
from tests import gif_ref


def palette(k, seed=0):
    """(k, 3) uint8, all entries different"""
    rng = np.random.default_rng(100 + seed)
    p = rng.permutation(1 << 12)[:k]
    return np.stack([(p & 15) * 17, ((p >> 4) & 15) * 17, (p >> 8) * 17], axis=1).astype(np.uint8)


def noise(h, w, levels, seed):
    return np.random.default_rng(seed).integers(0, levels, (h, w)).astype(np.uint8)


def waves(h, w, levels, seed=0):
    y, x = np.mgrid[0:h, 0:w]
    return ((np.sin(x / 7.0 + seed) + np.cos(y / 5.0)) * levels / 4 + levels / 2).clip(0, levels - 1).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------------------ streams
@functools.lru_cache(None)
def valid_streams():
    """name -> (indices (h, w) in stream order, code size, image data, the encoder's record)"""
    out = {}

    def add(name, indices, cs, **kw):
        rec = {}
        out[name] = (indices, cs, R.lzw_encode(indices, cs, record=rec, **kw), rec)

    add("flat", np.full((48, 64), 7, np.uint8), 8)                                # strings past 64 bytes, every code KwKwK
    add("noise_clear", noise(64, 96, 256, 1), 8)                                 # the table fills, a Clear follows
    add("noise_deferred", noise(64, 96, 256, 2), 8, clear_when_full=False)       # ... no Clear: 12-bit codes, frozen table
    for cs in (2, 3, 5, 7):
        add(f"cs{cs}", noise(64, 96, 1 << cs, 10 + cs), cs)
        add(f"cs{cs}_waves", waves(64, 96, 1 << cs, cs), cs)
    add("no_leading_clear", waves(31, 45, 256), 8, leading_clear=False)
    add("double_clear", noise(64, 96, 256, 3), 8, double_clear=True)
    add("no_eoi", waves(31, 45, 64, 1), 6, eoi=False)
    add("one_pixel", np.array([[3]], np.uint8), 2)
    add("deferred_waves", np.tile(waves(64, 96, 256, 2), (1, 1)) ^ noise(64, 96, 4, 5), 8, clear_when_full=False)
    long = np.concatenate([waves(20, 30, 128).reshape(-1), noise(1, 500, 128, 4).reshape(-1)])
    rec = {}
    out["too_many"] = (long[:600].reshape(20, 30), 7, R.lzw_encode(long, 7, record=rec), rec)       # 500 pixels behind the frame's last
    return out


@functools.lru_cache(None)
def damaged_streams():
    """name -> (w * h, code size, image data, status, produced): what the reference decoder says, asserted by the host test to be
    the status the case is built for"""
    w = waves(31, 45, 256)
    whole = R.lzw_encode(w, 8, eoi=False)
    cases = {
        "short_with_eoi": (31 * 45, 8, R.lzw_encode(w[:17], 8), R.SHORT),                           # End of Information after 17 rows
        "cut_without_eoi": (31 * 45, 8, whole[:len(whole) // 2], R.PAST_END),
        "empty": (31 * 45, 8, b"", R.PAST_END),
        "cut_noise": (64 * 96, 8, valid_streams()["noise_deferred"][2][:5000], R.PAST_END),         # cut at 12 bits, the table full
        "above_next_free": (100, 8, R.pack_codes([(256, 9), (5, 9), (6, 9), (300, 9), (1, 9)]), R.BAD_CODE),
        "above_clear_behind_clear": (100, 8, R.pack_codes([(256, 9), (5, 9), (6, 9), (256, 9), (258, 9), (1, 9)]), R.BAD_CODE),
        "above_clear_at_start": (100, 4, R.pack_codes([(18, 5), (1, 5)]), R.BAD_CODE),
        "eoi_at_start": (100, 4, R.pack_codes([(17, 5), (1, 5)]), R.SHORT),
    }
    out = {}
    for name, (n, cs, data, status) in cases.items():
        got, st = R.lzw_decode(data, cs, n)
        out[name] = (n, cs, data, status, len(got), st, got)
    return out


# ------------------------------------------------------------------------------------------------------------------------------ files
def random_file(seed):
    """a multi-frame file on a screen of up to 12 x 12: sub-rectangles, local and global tables, missing control extensions, all four
    disposals, transparency on any frame -> (bytes, width, height, frames, global_table, background)"""
    rng = np.random.default_rng(seed)
    W, H = int(rng.integers(1, 13)), int(rng.integers(1, 13))
    gk = int(rng.choice([0, 2, 4, 16]))
    global_table = palette(gk, seed) if gk else None
    background = int(rng.integers(0, 2)) if rng.random() < 0.5 else 0            # inside every table: the smallest has 2 entries
    frames = []
    for k in range(int(rng.integers(2, 7))):
        w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        left, top = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
        local = global_table is None or rng.random() < 0.4
        table = palette(int(rng.choice([2, 4, 8])), seed * 10 + k) if local else None
        entries = len(table) if local else gk
        control = rng.random() < 0.8
        frames.append(R.frame(rng.integers(0, entries, (h, w)), left, top, table,
                              transparent=int(rng.integers(0, entries)) if control and rng.random() < 0.6 else None,
                              disposal=int(rng.integers(0, 4)) if control else None, delay=int(rng.integers(0, 20)) if control else None,
                              interlace=bool(rng.random() < 0.3), control=control))
    return R.build(W, H, frames, global_table, background, loop=0 if rng.random() < 0.5 else None), W, H, frames, global_table, background


RANDOM_SEEDS = tuple(range(64))


def built(name):
    """the hand-built files -> (bytes, width, height, frames, global_table, background)"""
    g16, g256 = palette(16), palette(256, 1)
    if name == "interlaced_96x13":
        frames = [R.frame(waves(13, 96, 16), interlace=True)]
        return R.build(96, 13, frames, g16), 96, 13, frames, g16, 0
    if name == "interlaced_5x1":
        frames = [R.frame(np.array([[1, 2, 3, 4, 5]], np.uint8), interlace=True), R.frame(np.array([[5], [4], [3]], np.uint8), 1, 0, interlace=True)]
        return R.build(5, 3, frames, g16), 5, 3, frames, g16, 0
    if name == "six_rectangles":                                                  # streams of different lengths in one launch
        sizes = [(64, 96), (1, 1), (13, 40), (64, 3), (2, 96), (30, 30)]
        frames = [R.frame(noise(h, w, 256, 20 + i) if i % 2 else waves(h, w, 256, i), left=(96 - w) // 2, top=(64 - h) // 2,
                          transparent=7 if i in (2, 5) else None, disposal=(0, 1, 3, 2, 1, 0)[i], delay=5) for i, (h, w) in enumerate(sizes)]
        return R.build(96, 64, frames, g256, loop=3), 96, 64, frames, g256, 0
    if name == "dependent":                                                       # every frame needs its predecessors: disposal 3 and transparency
        frames = [R.frame(waves(24, 32, 16), delay=4)]
        for i in range(1, 7):
            frames.append(R.frame(noise(10, 12, 16, 40 + i), left=3 * i, top=2 * i, transparent=i, disposal=3 if i % 3 == 1 else 1, delay=4 + i % 2))
        return R.build(32, 24, frames, g16, loop=0), 32, 24, frames, g16, 0
    if name == "background_inside_table":
        data, W, H, frames, table, _ = built("background_beyond_table")
        return R.build(W, H, frames, table, background=2), W, H, frames, table, 2
    if name == "background_beyond_table":                                         # disposal 2 without transparency, background index 9 in 4-entry tables
        frames = [R.frame(noise(6, 6, 4, 50), disposal=2, delay=1, table=palette(4, 9)), R.frame(noise(3, 3, 4, 51), 1, 1, disposal=2, delay=1),
                  R.frame(noise(2, 2, 4, 52), 4, 4, delay=1, table=palette(4, 8))]
        return R.build(6, 6, frames, palette(4, 7), background=9), 6, 6, frames, palette(4, 7), 9
    if name == "gif87a_no_trailer":
        frames = [R.frame(waves(9, 11, 4), control=False), R.frame(noise(4, 5, 4, 53), 2, 3, control=False)]
        return R.build(11, 9, frames, palette(4, 3), version=b"GIF87a", trailer=False, comment=b"a comment " * 40), 11, 9, frames, palette(4, 3), 0
    raise KeyError(name)


BUILT = ("interlaced_96x13", "interlaced_5x1", "six_rectangles", "dependent", "background_inside_table", "gif87a_no_trailer")


def bad_index_file():
    """a frame whose second pixel is index 6 in a 4-entry table (code size 3 leaves room for it)"""
    frames = [R.frame(np.array([[0, 1, 2, 3]], np.uint8), code_size=3), R.frame(np.array([[1, 6]], np.uint8), 1, 0, code_size=3, delay=1),
              R.frame(np.array([[2]], np.uint8), code_size=3, delay=1)]
    return R.build(4, 1, frames, palette(4, 2)), frames


@functools.lru_cache(None)
def pillow_files():
    """files Pillow writes: name -> bytes"""
    from PIL import Image
    rng = np.random.default_rng(7)
    base = [Image.fromarray(np.stack([waves(40, 56, 256, k), waves(40, 56, 256, k + 3).T[:40, :40].repeat(2, 1)[:, :56], noise(40, 56, 256, k)], axis=-1), "RGB")
            for k in range(4)]
    moving = []
    for k in range(5):                                                            # a small square moving over a still background: Pillow crops the frames
        a = np.zeros((40, 56, 3), np.uint8) + np.array([30, 60, 90], np.uint8)
        a[5 + 4 * k:15 + 4 * k, 6 + 7 * k:16 + 7 * k] = (250, 40 * k, 10)
        moving.append(Image.fromarray(a, "RGB"))
    out = {}

    def save(name, frames, **kw):
        buf = io.BytesIO()
        frames[0].save(buf, "GIF", save_all=len(frames) > 1, append_images=frames[1:], **kw)
        out[name] = buf.getvalue()

    for d in range(4):
        save(f"disposal{d}", moving, disposal=d, duration=40, loop=0)
    save("photos", base, duration=[30, 40, 30, 30], loop=2)
    save("optimized", moving, optimize=True, duration=50)
    save("interlaced", base[:1], interlace=True)
    save("interlaced_clip", moving, interlace=True, disposal=2, duration=20)
    pal = [Image.fromarray(noise(20, 24, 5, k) + (np.mgrid[0:20, 0:24][1] > 4 * k + 4), "P") for k in range(4)]
    for im in pal:
        im.putpalette(palette(8, 4).reshape(-1).tolist())
    save("transparency", pal, transparency=0, disposal=2, duration=60, loop=0)
    save("transparency_keep", pal, transparency=3, disposal=1, duration=60)
    two = [Image.fromarray(np.roll(waves(17, 23, 2), 3 * k, axis=1), "P") for k in range(3)]
    for im in two:
        im.putpalette([10, 20, 30, 200, 210, 220])
    save("two_colours", two[:1])                                                  # a still: Pillow interlaces it
    save("two_colours_clip", two, duration=100)
    return out


@functools.lru_cache(None)
def own_writer_files():
    """encode_gif's container layout - 256-entry tables, a graphic control extension with disposal 1, whole frames, Clears between strips -
    built on the host: name -> (bytes, indices (n, H, W), palettes (1 | n, 256, 3), delays in centiseconds, loop)"""
    from emote_hack_amd import video_io as V
    out = {}
    for name, per_frame, strip_rows in (("global_strips8", False, 8), ("frame_strips8", True, 8), ("global_whole", False, None), ("frame_whole", True, None)):
        n, H, W = 3, 30, 44
        indices = np.stack([waves(H, W, 256, k) ^ noise(H, W, 8, 60 + k) for k in range(n)])
        palettes = np.stack([palette(256, 20 + k) for k in range(n if per_frame else 1)])
        delays = V.gif_delays(30, n)
        streams = [gif_ref.lzw_encode_strips(indices[k], strip_rows)[0] for k in range(n)]
        out[name] = (V.gif_container(W, H, palettes, streams, delays, loop=5), indices, palettes, delays, 5)
    return out
