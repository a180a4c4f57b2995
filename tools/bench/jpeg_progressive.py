"""Times the decoding of progressive JPEG files on the device (profiles/jpeg_progressive.md):

  progressive    Pillow's progressive file (libjpeg's default script: 10 scans at 4:2:0) through emo_jpeg_progressive_scan, one launch per
                 scan, then emo_jpeg_idct and emo_jpeg_rgb - without restart markers (a scan of a frame is ONE lane's walk) and
                 with restart_marker_rows=1 (one wavefront per row of units of every scan)
  baseline       Pillow's baseline file of the same picture through emo_jpeg_decode_bits / emo_jpeg_decode_segments and the same two
  pillow         PIL.Image.open(...).convert("RGB") of the progressive file (libjpeg, one host thread), host clock

on one 512 x 512 4:2:0 quality-90 still and on a clip of such frames (tools/bench/mjpeg.py's picture-like frames).  Before anything is
timed every variant is compared with Pillow: the frames must be equal.  The device side is timed on buffers uploaded once
(video_io._progressive_group_plan), device events around a run of back-to-back decodes, warmed up, several runs; the scans are also timed
one by one, each on the coefficients the scans before it leave (restored by a device copy in front of every call, which is timed alone
and subtracted).  decode_mjpeg as a user calls it - host parsing, the one copy, the launches, the status read - is timed with the host
clock, like Pillow.

    python tools/bench/jpeg_progressive.py [--reps 5] [--calls 20] [--frames 12] [--out FILE.md]
"""
import argparse
import io
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
    for _ in range(3):
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


def host_ms(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def pillow_file(pic, **kw):
    buf = io.BytesIO()
    Image.fromarray(pic).save(buf, format="JPEG", quality=90, subsampling=2, **kw)
    return buf.getvalue()


def pillow_decode(data):
    return np.array(Image.open(io.BytesIO(data)).convert("RGB"))


def progressive_decode(files, dev):
    """(a function that decodes the progressive files on buffers uploaded once: zero, one launch per scan, IDCT, colour; the plan)"""
    parsed = [V.parse_jpeg(d, progressive=True) for d in files]
    assert len({p.table_key() for p in parsed}) == 1 and parsed[0].layout.key == (3, 2, 2) and np.array_equal(parsed[0].quants[1], parsed[0].quants[2])
    plan = V._progressive_group_plan(parsed, list(range(len(parsed))), dev)
    H, W = parsed[0].height, parsed[0].width

    def run():
        plan["coefs"].zero_()
        for _, launch in plan["launches"]:
            launch()
        return ops.jpeg_rgb(*ops.jpeg_idct(plan["coefs"], plan["quant"], H, W), H, W)
    return run, plan


def baseline_decode(files, dev):
    """the same for baseline files: the entropy-decoding launch decode_mjpeg picks, IDCT, colour -> (all three, the first alone)"""
    parsed = [V.parse_jpeg(d, restart=True) for d in files]
    n, H, W = len(parsed), parsed[0].height, parsed[0].width
    n_mcu = ops.jpeg_mcus(H, W)
    sizes = np.array([len(p.scan) for p in parsed], np.int64)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    scan = torch.from_numpy(np.concatenate([p.scan for p in parsed] + [np.zeros(-int(sizes.sum()) % 4, np.uint8)])).to(dev)
    tables = torch.from_numpy(np.stack([V.huffman_decode_table(*s) for s in parsed[0].specs])).to(dev)
    quant = torch.from_numpy(parsed[0].quants.copy()).to(dev)
    assert all(p.specs == parsed[0].specs for p in parsed), "baseline files written without optimize= share the Annex K tables"
    if any(p.restart for p in parsed):
        off, first, blocks = [], [], []
        for f, p in enumerate(parsed):
            m0 = np.arange(len(p.intervals) - 1, dtype=np.int64) * (p.restart or n_mcu)
            off.append(start[f] + p.intervals[:-1])
            first.append((f * n_mcu + m0) * 6)
            blocks.append((np.minimum(m0 + (p.restart or n_mcu), n_mcu) - m0) * 6)
        off = torch.from_numpy(np.concatenate(off + [start[-1:]]).astype(np.int64)).to(dev)
        first, blocks = (torch.from_numpy(np.concatenate(x).astype(np.int32)).to(dev) for x in (first, blocks))
        entropy = lambda: ops.jpeg_decode_segments(scan, off, first, blocks, tables, n, n_mcu)
    else:
        off = torch.from_numpy(start).to(dev)
        entropy = lambda: ops.jpeg_decode_bits(scan, off, tables, n_mcu)
    return (lambda: ops.jpeg_rgb(*ops.jpeg_idct(entropy()[0], quant, H, W), H, W)), entropy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this benchmark measures on the GPU only")
    dev = torch.device("cuda")
    n, H, W = a.frames, 512, 512
    pics = picture_like(n, H, W).cpu().numpy()
    kinds = {"no restart markers": dict(), "restart_marker_rows=1": dict(restart_marker_rows=1)}
    f3 = lambda t: f"{t[0]:.3f} ({t[1]:.3f} - {t[2]:.3f})"
    rows = [f"device: {torch.cuda.get_device_name(0)}; Pillow {PIL.__version__}; frames of {H} x {W}, 4:2:0, quality 90, Pillow's writer (progressive: "
            f"libjpeg's default script of 10 scans); device events around {a.calls} back-to-back decodes on buffers uploaded once, {a.reps} runs "
            "(median, min - max); host-clock figures over the same number of runs; every variant's frames equal Pillow's byte for byte.", ""]
    per_scan = None
    for count in (1, n):
        rows += [f"{count} frame{'s' if count > 1 else ''}:", "",
                 "| files | bytes per frame, progressive / baseline | progressive on the device, ms: 10 scan launches + IDCT + colour | the 10 scan launches alone "
                 "| baseline on the device, ms: entropy launch + IDCT + colour | its entropy launch alone | decode_mjpeg(progressive=True) as called, host "
                 "clock, ms | decode_mjpeg on the baseline files, host clock, ms | Pillow on the progressive files, host, ms |", "|---|---|---|---|---|---|---|---|---|"]
        for label, kw in kinds.items():
            prog = [pillow_file(p, progressive=True, **kw) for p in pics[:count]]
            base = [pillow_file(p, **kw) for p in pics[:count]]
            want = np.stack([pillow_decode(d) for d in prog])
            assert np.array_equal(want, np.stack([pillow_decode(d) for d in base]))
            run, plan = progressive_decode(prog, dev)
            run_base, entropy = baseline_decode(base, dev)
            assert np.array_equal(run().cpu().numpy(), want) and np.array_equal(run_base().cpu().numpy(), want), label
            assert np.array_equal(V.decode_mjpeg(prog, progressive=True).cpu().numpy(), want) and not plan["status"].cpu().numpy().any()

            def scans_only():
                plan["coefs"].zero_()
                for _, launch in plan["launches"]:
                    launch()
            rows.append(f"| {label} | {sum(map(len, prog)) / count:.0f} / {sum(map(len, base)) / count:.0f} | {f3(device_ms(run, a.reps, a.calls))} | "
                        f"{f3(device_ms(scans_only, a.reps, a.calls))} | {f3(device_ms(run_base, a.reps, a.calls))} | {f3(device_ms(entropy, a.reps, a.calls))} | "
                        f"{f3(host_ms(lambda: V.decode_mjpeg(prog, progressive=True), a.reps))} | {f3(host_ms(lambda: V.decode_mjpeg(base), a.reps))} | "
                        f"{f3(host_ms(lambda: [pillow_decode(d) for d in prog], a.reps))} |")
            if count == 1:
                # every scan alone, on the coefficients the scans before it leave
                coefs = plan["coefs"]
                coefs.zero_()
                before = []
                for _, launch in plan["launches"]:
                    before.append(coefs.clone())
                    launch()
                spare = torch.empty_like(coefs)
                copy = device_ms(lambda: spare.copy_(before[0]), a.reps, a.calls)
                split = []
                for (sc, launch), snap in zip(plan["launches"], before):
                    def one(launch=launch, snap=snap):
                        coefs.copy_(snap)
                        launch()
                    t = device_ms(one, a.reps, a.calls)
                    parsed = V.parse_jpeg(prog[0], progressive=True).scans[len(split)]
                    split.append((sc, len(parsed.scan), len(parsed.intervals) - 1, t))
                per_scan = per_scan or []
                per_scan.append((label, copy, split))
        rows.append("")
    for label, copy, split in per_scan:
        rows += [f"the scans of the one still one by one, {label} (each launch behind a device copy that restores the coefficients it starts from; the "
                 f"copy alone takes {copy[0]:.3f} ms and is subtracted):", "",
                 "| scan | components | Ss .. Se | Ah / Al | bytes | segments (wavefronts) | ms |", "|---|---|---|---|---|---|---|"]
        for k, (sc, size, segs, t) in enumerate(split):
            rows.append(f"| {k} | {','.join(map(str, sc.components))} | {sc.Ss} .. {sc.Se} | {sc.Ah} / {sc.Al} | {size} | {segs} | "
                        f"{max(t[0] - copy[0], 0.0):.3f} ({max(t[1] - copy[0], 0.0):.3f} - {max(t[2] - copy[0], 0.0):.3f}) |")
        rows.append(f"| all | | | | {sum(s[1] for s in split)} | {sum(s[2] for s in split)} | {sum(max(s[3][0] - copy[0], 0.0) for s in split):.3f} |")
        rows.append("")
    text = "\n".join(rows)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
