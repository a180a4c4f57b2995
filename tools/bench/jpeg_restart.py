"""Times the decoding of Motion-JPEG frames with and without restart intervals (profiles/jpeg_restart.md):

  by hand    a file without restart markers on the frame-serial path, called launch by launch: parse_jpeg, one copy, emo_jpeg_decode_bits
             (one workgroup per frame, one lane walks the frame), emo_jpeg_idct, emo_jpeg_rgb, one status read
  plain      the same file through decode_mjpeg (the same launches: a clip without restart intervals keeps that path)
  row        encode_mjpeg(restart_interval="row") through decode_mjpeg: one wavefront per row of MCUs
  4          encode_mjpeg(restart_interval=4) through decode_mjpeg: one wavefront per 4 MCUs
  pillow     PIL.Image.open(...).convert("RGB") per frame (libjpeg, one host thread), then the copy of the uint8 frames to the device

on 1 frame and on a clip of 512 x 512 frames at one quality (tools/bench/mjpeg.py's picture-like frames).  Device events around each path
(every path ends on the device; the events also see the host work a path does between its launches), every variant warmed up, the
variants alternate inside each repetition; mean and min - max over the repetitions.  The entropy-decoding launch of each variant is
timed on its own as well (a file without markers also as ONE segment per frame, which decode_mjpeg does only for such a frame among
frames that have markers), and the files' sizes are listed: the markers and the padding of every interval cost bytes.  Before anything
is timed every variant's frames are compared with Pillow's: they must be equal.

    python tools/bench/jpeg_restart.py [--reps 10] [--frames 48] [--quality 90] [--out FILE.md]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from emote_hack_amd import ops, video_io as V            # noqa: E402
from mjpeg import DEV, picture_like                      # noqa: E402  (tools/bench/mjpeg.py: the encoder's benchmark, the same frames)
from mjpeg_decode import pil_decode_to_device            # noqa: E402


def upload(parsed):
    """(scan, frame offsets, tables, quantisers) of frames that share their tables, on the device in one copy each"""
    sizes = np.array([len(p.scan) for p in parsed], np.int64)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).to(DEV)
    scan = torch.from_numpy(np.concatenate([p.scan for p in parsed] + [np.zeros(-int(sizes.sum()) % 4, np.uint8)])).to(DEV)
    tables = torch.from_numpy(np.stack([V.huffman_decode_table(*s) for s in parsed[0].specs])).to(DEV)
    return scan, offsets, tables, torch.from_numpy(parsed[0].quants.copy()).to(DEV)


def decode_frame_serial(jpegs):
    """what decode_mjpeg does for files without restart markers, launch by launch: emo_jpeg_decode_bits, one workgroup per frame"""
    parsed = [V.parse_jpeg(j) for j in jpegs]
    H, W = parsed[0].height, parsed[0].width
    scan, offsets, tables, quant = upload(parsed)
    coefs, status = ops.jpeg_decode_bits(scan, offsets, tables, ops.jpeg_mcus(H, W))
    rgb = ops.jpeg_rgb(*ops.jpeg_idct(coefs, quant, H, W), H, W)
    assert not status.cpu().numpy().any()
    return rgb


def segment_launch(jpegs):
    """the entropy-decoding launch of decode_mjpeg on these files, on buffers uploaded once -> a callable"""
    parsed = [V.parse_jpeg(j, restart=True) for j in jpegs]
    n, n_mcu = len(parsed), ops.jpeg_mcus(parsed[0].height, parsed[0].width)
    scan, offsets, tables, _ = upload(parsed)
    seg_offsets, first, blocks = [], [], []
    for f, p in enumerate(parsed):
        m0 = np.arange(len(p.intervals) - 1, dtype=np.int64) * (p.restart or n_mcu)
        seg_offsets.append(int(offsets[f]) + p.intervals[:-1])
        first.append((f * n_mcu + m0) * 6)
        blocks.append((np.minimum(m0 + (p.restart or n_mcu), n_mcu) - m0) * 6)
    seg_offsets = torch.from_numpy(np.concatenate(seg_offsets + [[int(offsets[-1])]]).astype(np.int64)).to(DEV)
    first, blocks = (torch.from_numpy(np.concatenate(x).astype(np.int32)).to(DEV) for x in (first, blocks))
    return (lambda: ops.jpeg_decode_segments(scan, seg_offsets, first, blocks, tables, n, n_mcu)), int(first.numel())


def frame_launch(jpegs):
    parsed = [V.parse_jpeg(j) for j in jpegs]
    scan, offsets, tables, _ = upload(parsed)
    n_mcu = ops.jpeg_mcus(parsed[0].height, parsed[0].width)
    return lambda: ops.jpeg_decode_bits(scan, offsets, tables, n_mcu)


def event_timed(variants, reps):
    """ms of every variant, device events, the variants alternating inside each repetition"""
    for fn in variants.values():
        for _ in range(2):
            fn()
    out = {k: [] for k in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b))
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
    files = {"plain": V.encode_mjpeg(frames, q), "row": V.encode_mjpeg(frames, q, restart_interval="row"),
             "4": V.encode_mjpeg(frames, q, restart_interval=4)}
    want = pil_decode_to_device(files["plain"])
    for name, jpegs in files.items():
        assert torch.equal(V.decode_mjpeg(jpegs), want) and torch.equal(pil_decode_to_device(jpegs), want), name
    assert torch.equal(decode_frame_serial(files["plain"]), want)
    size = {k: sum(map(len, v)) / n for k, v in files.items()}
    rows = [f"device: {torch.cuda.get_device_name(0)}; frames of {H} x {W}, quality {q}, 4:2:0; {a.reps} repetitions, device events, every path ends "
            "on the device; every variant's frames equal Pillow's byte for byte", "",
            "| file | bytes per frame | over the plain file | restart intervals per frame |", "|---|---|---|---|"]
    for k, label in (("plain", "no restart interval"), ("row", 'restart_interval="row" (32 MCUs)'), ("4", "restart_interval=4")):
        rows.append(f"| {label} | {size[k]:.0f} | {100.0 * (size[k] / size['plain'] - 1.0):+.2f} % | {len(V.parse_jpeg(files[k][0], restart=True).intervals) - 1} |")
    rows.append("")
    for count in (1, n):
        clip = {k: v[:count] for k, v in files.items()}
        paths = {"the frame-serial path by hand: plain file, emo_jpeg_decode_bits (one workgroup per frame)": lambda: decode_frame_serial(clip["plain"]),
                 "decode_mjpeg, plain file (emo_jpeg_decode_bits as well)": lambda: V.decode_mjpeg(clip["plain"]),
                 'decode_mjpeg, restart_interval="row"': lambda: V.decode_mjpeg(clip["row"]),
                 "decode_mjpeg, restart_interval=4": lambda: V.decode_mjpeg(clip["4"]),
                 "PIL.Image.open per frame (libjpeg, one thread) + the copy of the uint8 frames to the device": lambda: pil_decode_to_device(clip["plain"])}
        t = event_timed(paths, a.reps)
        rows += [f"{count} frame{'s' if count > 1 else ''}, the whole path (host parsing, one copy, three launches, one status read):", "",
                 "| path | ms in all, mean | min | max | ms per frame, mean |", "|---|---|---|---|---|"]
        rows += [f"| {k} | {statistics.mean(ms):.3f} | {min(ms):.3f} | {max(ms):.3f} | {statistics.mean(ms) / count:.3f} |" for k, ms in t.items()]
        launches, segs = {"emo_jpeg_decode_bits, plain file": frame_launch(clip["plain"])}, {}
        for k, label in (("plain", "plain file"), ("row", 'restart_interval="row"'), ("4", "restart_interval=4")):
            fn, n_seg = segment_launch(clip[k])
            launches[f"emo_jpeg_decode_segments, {label} ({n_seg} segments)"] = fn
        coefs = [fn()[0] for fn in launches.values()]
        assert all(torch.equal(c, coefs[0]) for c in coefs)                      # restart intervals do not change the coefficients
        t = event_timed(launches, a.reps)
        rows += ["", f"the entropy-decoding launch alone on these {count} frame{'s' if count > 1 else ''}:", "", "| launch | ms, mean | min | max |",
                 "|---|---|---|---|"]
        rows += [f"| {k} | {statistics.mean(ms):.3f} | {min(ms):.3f} | {max(ms):.3f} |" for k, ms in t.items()] + [""]
    text = "\n".join(rows)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
