"""Times the decoding of ONE 512 x 512 JPEG frame per layout - 4:2:0, 4:2:2, 4:4:4, grey - with and without restart intervals of one
MCU row, device path against what a user had before it (profiles/jpeg_layouts.md):

  new   emote_hack_amd.video_io.decode_mjpeg([file]): marker parsing and byte unstuffing on the host, ONE host-to-device copy, three
        launches (emo_jpeg_decode_bits / emo_jpeg_decode_segments, emo_jpeg_idct, emo_jpeg_rgb), one read of the status; the frame ends
        on the device
  old   PIL.Image.open(...).convert("RGB") (libjpeg, one host thread), then the host-to-device copy of the uint8 frame

on the same files, which Pillow writes from tools/bench/mjpeg.py's picture-like frame.  Host clock around work that ends in a device
synchronise; every variant is warmed up, the two sides alternate inside each repetition, and the median with the min - max spread over
the repetitions is reported.  Before anything is timed the two paths' frames are compared: they must be equal.

    python tools/bench/jpeg_layouts.py [--reps 20] [--quality 90] [--out FILE.md]
"""
import argparse
import io
import os
import statistics
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from emote_hack_amd import video_io as V                 # noqa: E402
from mjpeg import DEV, picture_like, timed               # noqa: E402  (tools/bench/mjpeg.py: the encoder's benchmark, the same frames)

SUBSAMPLING = {"4:2:0": 2, "4:2:2": 1, "4:4:4": 0}


def pillow_file(frame, name, quality, rows):
    buf = io.BytesIO()
    if name == "grey":
        Image.fromarray(np.ascontiguousarray(frame[..., 1])).save(buf, format="JPEG", quality=quality, restart_marker_rows=rows)
    else:
        Image.fromarray(frame).save(buf, format="JPEG", quality=quality, subsampling=SUBSAMPLING[name], restart_marker_rows=rows)
    return buf.getvalue()


def pil_decode_to_device(data):
    return torch.from_numpy(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))).to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this benchmark measures on the GPU only")
    H = W = 512
    frame = picture_like(1, H, W)[0].cpu().numpy()
    rows = [f"device: {torch.cuda.get_device_name(0)}; one frame of {H} x {W}, quality {a.quality}, written by Pillow; {a.reps} repetitions, host clock, "
            "every path ends on the device after a synchronise; the two paths' frames are equal byte for byte", "",
            "| layout | restart interval | file bytes | segments | decode_mjpeg ms, median | min | max | Pillow + upload ms, median | min | max |",
            "|---|---|---|---|---|---|---|---|---|---|"]
    for name in ("4:2:0", "4:2:2", "4:4:4", "grey"):
        for restart_rows in (0, 1):
            data = pillow_file(frame, name, a.quality, restart_rows)
            assert torch.equal(V.decode_mjpeg([data])[0], pil_decode_to_device(data)), (name, restart_rows)
            p = V.parse_jpeg(data, restart=True, layouts=True)
            t = timed({"new": lambda: V.decode_mjpeg([data]), "old": lambda: pil_decode_to_device(data)}, a.reps)
            cells = [f"{f(t[k]):.3f}" for k in ("new", "old") for f in (statistics.median, min, max)]
            rows.append(f"| {name} | {'one MCU row (' + str(p.restart) + ' MCUs)' if p.restart else 'none'} | {len(data)} | {len(p.intervals) - 1} | "
                        + " | ".join(cells) + " |")
    text = "\n".join(rows)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
