"""Times the resize of a clip's frames, device path against what a user had before it (profiles/image_resize.md):

  new   emote_hack_amd.video_io.resize_frames on frames that are on the device: emo_image_resize, a horizontal and a vertical launch
  old   Image.fromarray(f).resize((width, height), filter) per frame (Pillow, one host thread), frames on the host

on the same frames: 12 of 1080 x 1920 to 512 x 512 (a driving video at the size the pipeline is benchmarked at), picture-like
(tools/bench/mjpeg.py).  Before anything is timed the two results are compared: they must be equal.  The device side is timed with device
events around a run of back-to-back calls (one call is a fraction of a millisecond), warmed up, several runs; the two passes are also
timed alone, the vertical one on the intermediate image.  Pillow is timed with the host clock.

    python tools/bench/image_resize.py [--reps 5] [--calls 200] [--frames 12] [--out FILE.md]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import PIL
import torch
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from emote_hack_amd import ops, video_io as V            # noqa: E402
from mjpeg import picture_like                           # noqa: E402  (tools/bench/mjpeg.py: the same picture-like frames)


def device_ms(fn, reps, calls):
    """ms per call over `calls` back-to-back calls between two device events, `reps` times -> (median, min, max)"""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this benchmark measures on the GPU only")
    n, H, W, h, w = a.frames, 1080, 1920, 512, 512
    frames = picture_like(n, H, W)
    host = frames.cpu().numpy()
    moved = n * (H * W * 3 + 2 * H * w * 3 + h * w * 3)
    rows = [f"device: {torch.cuda.get_device_name(0)}; Pillow {PIL.__version__}; {n} frames of {H} x {W} -> {h} x {w}; device events around {a.calls} "
            f"back-to-back calls, {a.reps} runs (median, min - max); Pillow on one host thread, host clock, {a.reps} runs; the two results are "
            f"equal byte for byte.  The two passes read and write {moved / 1e6:.1f} MB (frames in, the intermediate {n} x {H} x {w} out and in, "
            "frames out).", "",
            "| filter | table width (ksize), x / y | emo_image_resize, ms per call | horizontal pass alone | vertical pass alone | GB/s over both passes "
            "| Pillow on the host, ms | Pillow / device |", "|---|---|---|---|---|---|---|---|"]
    for name in ("bilinear", "bicubic", "lanczos"):
        flt = getattr(Image.Resampling, name.upper())
        pillow = lambda: np.stack([np.array(Image.fromarray(f).resize((w, h), flt)) for f in host])
        got = V.resize_frames(frames, (w, h), name)
        assert np.array_equal(got.cpu().numpy(), pillow()), name
        xt, yt = V._device_resize_taps(W, w, name, str(frames.device)), V._device_resize_taps(H, h, name, str(frames.device))
        out, mid = torch.empty(n, h, w, 3, device=frames.device, dtype=torch.uint8), torch.empty(n, H, w, 3, device=frames.device, dtype=torch.uint8)
        both = device_ms(lambda: ops.image_resize(frames, h, w, xt, yt, out=out), a.reps, a.calls)
        hor = device_ms(lambda: ops.image_resize(frames, H, w, xt, None, out=mid), a.reps, a.calls)
        ver = device_ms(lambda: ops.image_resize(mid, h, w, None, yt, out=out), a.reps, a.calls)
        pil = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            pillow()
            pil.append((time.perf_counter() - t0) * 1e3)
        f3 = lambda t: f"{t[0]:.3f} ({t[1]:.3f} - {t[2]:.3f})"
        rows.append(f"| {name} | {xt[1].shape[1]} / {yt[1].shape[1]} | {f3(both)} | {f3(hor)} | {f3(ver)} | {moved / both[0] / 1e6:.0f} | "
                    f"{statistics.median(pil):.1f} ({min(pil):.1f} - {max(pil):.1f}) | {statistics.median(pil) / both[0]:.0f}x |")
    text = "\n".join(rows)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
