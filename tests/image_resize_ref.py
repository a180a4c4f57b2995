"""Numpy restatement of Pillow's resize of 8-bit images (Resample.c: ImagingResampleHorizontal_8bpc, ImagingResampleVertical_8bpc) on the
tables of emote_hack_amd.video_io.resize_taps: a horizontal pass to 8-bit pixels, then a vertical pass over those; int64 sums from
1 << 21, `>> 22`, a clip to 0 .. 255.  A pass whose axis keeps its size is skipped, as ImagingResample skips it.  Shared by the host and
the device tests."""
import numpy as np

from emote_hack_amd import video_io as V

FILTERS = ("box", "bilinear", "hamming", "bicubic", "lanczos")
# (input h x w, output h x w): both ways on both axes, one axis alone, the same size, a 1-pixel-wide strip, a strong shrink
SHAPES = [((37, 53), (64, 64)), ((64, 64), (24, 40)), ((19, 128), (19, 31)), ((50, 7), (8, 16)), ((16, 16), (16, 16)), ((3, 5), (32, 8)),
          ((97, 61), (8, 8))]


def pillow_filter(name):
    from PIL import Image
    return getattr(Image.Resampling, name.upper())


def pillow_resize(frame, h, w, name=None):
    """Pillow itself: Image.fromarray(frame).resize((w, h)[, filter])"""
    from PIL import Image
    im = Image.fromarray(frame)
    return np.array(im.resize((w, h)) if name is None else im.resize((w, h), pillow_filter(name)))


def resample_axis(x, axis, bounds, coef):
    """one pass along `axis` of a uint8 array with the (bounds, coef) of that axis"""
    x = np.moveaxis(x, axis, 0).astype(np.int64)
    out = np.empty((len(bounds),) + x.shape[1:], np.uint8)
    for o, (first, count) in enumerate(bounds):
        acc = np.tensordot(coef[o, :count].astype(np.int64), x[first:first + count], axes=1) + (1 << (V.RESIZE_PRECISION_BITS - 1))
        out[o] = np.clip(acc >> V.RESIZE_PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(frames, h, w, name="bicubic"):
    """(..., H, W, 3) uint8 -> (..., h, w, 3) uint8"""
    frames = np.asarray(frames)
    H, W = frames.shape[-3], frames.shape[-2]
    if W != w:
        frames = resample_axis(frames, frames.ndim - 2, *V.resize_taps(W, w, name))
    if H != h:
        frames = resample_axis(frames, frames.ndim - 3, *V.resize_taps(H, h, name))
    return frames.copy()


def make_frames(content, n, H, W, seed=0):
    """uint8 (n, H, W, 3) test frames: "noise"; "checker" (0 / 255 per pixel: the negative lobes of bicubic and lanczos overshoot on both
    sides, so the clamp decides); "white" (255 everywhere: the rounding must give 255 back) and "black" """
    if content == "noise":
        return np.random.default_rng(seed + 1000 * H + W).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    if content == "checker":
        yy, xx = np.mgrid[0:H, 0:W]
        board = (((yy + xx) & 1) * 255).astype(np.uint8)
        return np.ascontiguousarray(np.broadcast_to(board[None, :, :, None], (n, H, W, 3)))
    if content in ("white", "black"):
        return np.full((n, H, W, 3), 255 if content == "white" else 0, np.uint8)
    raise ValueError(content)
