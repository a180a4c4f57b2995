"""Times the decoding of a Motion-JPEG clip's frames, device path against what a user had before it (profiles/mjpeg_decode.md):

  new   emote_hack_amd.video_io.decode_mjpeg: marker parsing and byte unstuffing on the host, ONE host-to-device copy of the scans,
        emo_jpeg_decode_bits, emo_jpeg_idct, emo_jpeg_rgb, one read of the frames' status; the frames end on the device
  old   PIL.Image.open(...).convert("RGB") per frame (libjpeg, one host thread), then the host-to-device copy of the uint8 frames

on the same files: a clip of 512 x 512 frames (the size the pipeline is benchmarked at) encoded by encode_mjpeg, then one frame of it.
The frames are tools/bench/mjpeg.py's picture-like ones.  Host clock around work that ends in a device synchronise (both paths end on the
device); every variant is warmed up, the two sides alternate inside each repetition, and the median with the min - max spread over the
repetitions is reported.  The three kernels are timed one by one with device events on the clip's own buffers.  Before anything is
timed the two paths' frames are compared: they must be equal.

    python tools/bench/mjpeg_decode.py [--reps 10] [--frames 48] [--quality 90] [--out FILE.md]
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
from emote_hack_amd import ops, video_io as V            # noqa: E402
from mjpeg import DEV, picture_like, timed               # noqa: E402  (tools/bench/mjpeg.py: the encoder's benchmark, the same frames)


def pil_decode_to_device(jpegs):
    host = np.stack([np.asarray(Image.open(io.BytesIO(j)).convert("RGB")) for j in jpegs])
    return torch.from_numpy(host).to(DEV)


def kernel_split(jpegs, reps):
    """ms of each of the three launches on the clip's own buffers, device events, (median, min, max) per kernel"""
    parsed = [V.parse_jpeg(j) for j in jpegs]
    H, W, n = parsed[0].height, parsed[0].width, len(parsed)
    sizes = np.array([len(p.scan) for p in parsed], np.int64)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).to(DEV)
    scan = np.concatenate([p.scan for p in parsed] + [np.zeros(-int(sizes.sum()) % 4, np.uint8)])
    scan = torch.from_numpy(scan).to(DEV)
    tables = torch.from_numpy(np.stack([V.huffman_decode_table(*s) for s in parsed[0].specs])).to(DEV)
    quant = torch.from_numpy(parsed[0].quants.copy()).to(DEV)
    n_mcu = ops.jpeg_mcus(H, W)
    coefs, _ = ops.jpeg_decode_bits(scan, offsets, tables, n_mcu)
    y, c = ops.jpeg_idct(coefs, quant, H, W)
    steps = {"emo_jpeg_decode_bits": lambda: ops.jpeg_decode_bits(scan, offsets, tables, n_mcu),
             "emo_jpeg_idct": lambda: ops.jpeg_idct(coefs, quant, H, W),
             "emo_jpeg_rgb": lambda: ops.jpeg_rgb(y, c, H, W)}
    out = {}
    for name, fn in steps.items():
        for _ in range(2):
            fn()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        out[name] = (statistics.median(ms), min(ms), max(ms))
    return out, int(sizes.sum())


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
    jpegs = V.encode_mjpeg(picture_like(n, H, W), q)
    assert torch.equal(V.decode_mjpeg(jpegs), pil_decode_to_device(jpegs))
    rows = [f"device: {torch.cuda.get_device_name(0)}; frames of {H} x {W}, quality {q}, 4:2:0, {sum(map(len, jpegs)) / n:.0f} bytes per file "
            f"(raw: {H * W * 3}); {a.reps} repetitions, host clock, every path ends on the device after a synchronise; the two paths' frames "
            "are equal byte for byte", ""]
    for count in (n, 1):
        clip = jpegs[:count]
        t = timed({"decode_mjpeg (host parsing, one copy of the scans, three launches, one status read)": lambda: V.decode_mjpeg(clip),
                   "  of which: parse_jpeg per frame on the host": lambda: [V.parse_jpeg(j) for j in clip],
                   "PIL.Image.open per frame (libjpeg, one thread) + the copy of the uint8 frames to the device": lambda: pil_decode_to_device(clip)},
                  a.reps)
        rows += [f"{count} frame{'s' if count > 1 else ''}:", "", "| path | ms per frame, median | min | max | ms in all, median |", "|---|---|---|---|---|"]
        for name, ms in t.items():
            rows.append(f"| {name} | {statistics.median(ms) / count:.3f} | {min(ms) / count:.3f} | {max(ms) / count:.3f} | {statistics.median(ms):.2f} |")
        split, scan_bytes = kernel_split(clip, a.reps)
        rows += ["", f"the three launches on these {count} frame{'s' if count > 1 else ''} ({scan_bytes} scan bytes), device events:", "",
                 "| kernel | ms, median | min | max |", "|---|---|---|---|"]
        rows += [f"| {k} | {med:.3f} | {lo:.3f} | {hi:.3f} |" for k, (med, lo, hi) in split.items()] + [""]
    text = "\n".join(rows)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
