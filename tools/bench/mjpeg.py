"""Times the JPEG encoding of a clip's 8-bit frames, device path against what a user had before it (profiles/mjpeg_encode.md):

  new   emote_hack_amd.video_io.encode_mjpeg: emo_jpeg_blocks, emo_jpeg_count_bits, emo_jpeg_emit_bits, one device-to-host copy of the
        compressed streams, then padding / byte stuffing / headers per frame on the host
  old   a device-to-host copy of the uint8 frames, then PIL.Image.save(format="JPEG", quality=q, subsampling=2) per frame (libjpeg, one
        host thread)

at 512 x 512, the size the pipeline is benchmarked at.  The frames are synthetic but picture-like (a smooth colour field, some texture,
mild sensor noise), so the compressed size per frame is in the range of a photograph's; it is reported with the timings, as is Pillow's.
Host clock around work that ends on the host (both paths do); every variant is warmed up, the two sides alternate inside each repetition,
and the median with the min - max spread over the repetitions is reported.  Before anything is timed, Pillow decodes a device-encoded
frame and the two files' PSNR against the source is compared.

    python tools/bench/mjpeg.py [--reps 10] [--frames 48] [--quality 90] [--out FILE.md]
"""
import argparse
import io
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from emote_hack_amd import video_io as V                 # noqa: E402

DEV = "cuda"


def picture_like(n, H, W, seed=0):
    """(n, H, W, 3) uint8 on the device: low-pass noise at two scales plus fine noise, drifting from frame to frame"""
    g = torch.Generator().manual_seed(seed)
    up = lambda t: torch.nn.functional.interpolate(t, size=(H, W), mode="bicubic", align_corners=False)
    coarse, mid = torch.randn(1, 3, 6, 6, generator=g), torch.randn(1, 3, 48, 48, generator=g)
    frames = []
    for i in range(n):
        coarse = coarse + 0.05 * torch.randn(1, 3, 6, 6, generator=g)
        mid = mid + 0.05 * torch.randn(1, 3, 48, 48, generator=g)
        x = 128 + 60 * up(coarse) + 14 * up(mid) + 2.0 * torch.randn(1, 3, H, W, generator=g)
        frames.append(x[0].permute(1, 2, 0))
    return torch.stack(frames).clamp(0, 255).to(torch.uint8).to(DEV).contiguous()


def pil_jpeg(frame, quality):
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG", quality=quality, subsampling=2)
    return buf.getvalue()


def psnr(a, b):
    return 10.0 * np.log10(255.0 ** 2 / max(float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)), 1e-12))


def timed(variants, reps):
    for fn in variants.values():
        for _ in range(2):
            fn()
    out = {k: [] for k in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this benchmark measures on the GPU only")
    n, H, W, q = a.frames, 512, 512, a.quality
    frames = picture_like(n, H, W)
    new = lambda: V.encode_mjpeg(frames, q)
    old = lambda: [pil_jpeg(f, q) for f in frames.cpu().numpy()]

    def device_part():
        V.encode_streams(frames, q)
        torch.cuda.synchronize()
    copy_only = lambda: frames.cpu()
    mine, theirs, host = new(), old(), frames.cpu().numpy()
    decoded = [np.asarray(Image.open(io.BytesIO(j)).convert("RGB")) for j in (mine[0], theirs[0])]
    assert decoded[0].shape == (H, W, 3)
    p_new, p_old = psnr(decoded[0], host[0]), psnr(decoded[1], host[0])
    assert p_new > p_old - 0.25, (p_new, p_old)
    t = timed({"encode_mjpeg (device encode, one copy of the streams, host framing)": new,
               "  of which: three launches + the read of the frame totals, synchronised": device_part,
               "frames.cpu() + PIL.Image.save per frame (libjpeg, one thread)": old,
               "  of which: the device-to-host copy of the uint8 frames": copy_only}, a.reps)
    rows = [f"device: {torch.cuda.get_device_name(0)}; {n} frames of {H} x {W}, quality {q}, 4:2:0; {a.reps} repetitions, host clock, every path ends "
            "on the host", "",
            f"bytes per frame: device {sum(map(len, mine)) / n:.0f}, Pillow {sum(map(len, theirs)) / n:.0f} (raw: {H * W * 3}); PSNR of frame 0 against "
            f"its source: device {p_new:.2f} dB, Pillow {p_old:.2f} dB", "",
            "| path | ms per frame, median | min | max | ms per clip, median |", "|---|---|---|---|---|"]
    for name, ms in t.items():
        rows.append(f"| {name} | {statistics.median(ms) / n:.3f} | {min(ms) / n:.3f} | {max(ms) / n:.3f} | {statistics.median(ms):.1f} |")
    text = "\n".join(rows)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
