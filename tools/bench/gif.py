"""Times the GIF encoding of a clip's 8-bit frames, stage by stage, beside Pillow on the host (profiles/gif_encode.md):

  new   emote_hack_amd.video_io.encode_gif: emo_gif_histogram, the read of the histogram and the median cut on the host, emo_gif_map,
        emo_gif_lzw_count, the read of the frame totals, emo_gif_lzw_emit, one device-to-host copy of the code streams, the container
  old   a device-to-host copy of the uint8 frames, then PIL's `save(format="GIF", save_all=True)` of the same frames (its own quantiser
        and a serial LZW coder, one host thread)

at 512 x 512, the size the pipeline is benchmarked at, for 12 and for 48 frames, on two kinds of content: `noisy`, the synthetic clip of
tests/gif_ref.py (waves, ramps, N(0, 6) noise: few repeats, long dictionaries), and `portrait`, a flat background behind a textured,
moving oval (most pixels in a few bins, long strings).  The kernels are timed with device events after a warm-up, the host stages and the
whole calls with the host clock around work that ends on the host; medians with the min - max spread.  A second table gives the LZW payload
and the time of the two LZW kernels for strip_rows in 1, 4, 8, 16, 32 and None (one stream per frame).  Before anything is timed, Pillow
decodes the device's file and every frame must equal palette[indices].

    python tools/bench/gif.py [--reps 10] [--out FILE.md]
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
from emote_hack_amd import ops                           # noqa: E402
from emote_hack_amd import video_io as V                 # noqa: E402

DEV = "cuda"
STRIPS = (1, 4, 8, 16, 32, None)


def noisy(n, H, W, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.zeros((n, H, W, 3), np.float32)
    for k in range(n):
        out[k, ..., 0] = 128 + 100 * np.sin(x / (9 + k) + y / 17)
        out[k, ..., 1] = 128 + 90 * np.cos(y / 11 - 0.3 * k)
        out[k, ..., 2] = 0.6 * 255 * x / W + 0.4 * 255 * y / H
    out += rng.normal(0, 6, out.shape).astype(np.float32)
    out[:, H // 4:H // 2, W // 4:W // 2] = np.array([230, 180, 150], np.float32) + rng.normal(0, 3, (n, H // 4, W // 4, 3)).astype(np.float32)
    return np.clip(out, 0, 255).astype(np.uint8)


def portrait(n, H, W, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.empty((n, H, W, 3), np.uint8)
    skin = np.array([224, 172, 140], np.float32)
    for k in range(n):
        cx, cy = W / 2 + 6 * np.sin(k / 3), H / 2 + 4 * np.cos(k / 5)
        inside = ((x - cx) / (0.22 * W)) ** 2 + ((y - cy) / (0.3 * H)) ** 2 < 1
        face = skin + 25 * np.sin(x / 13 + k / 4)[..., None] + rng.normal(0, 3, (H, W, 3))
        out[k] = np.where(inside[..., None], np.clip(face, 0, 255), np.array([32, 48, 96], np.float32)).astype(np.uint8)
    return out


def pil_gif(host, delays):
    ims = [Image.fromarray(f) for f in host]
    buf = io.BytesIO()
    ims[0].save(buf, format="GIF", save_all=True, append_images=ims[1:], duration=[10 * d for d in delays], loop=0)
    return buf.getvalue()


def stats(ms):
    return f"{statistics.median(ms):.3f} | {min(ms):.3f} | {max(ms):.3f}"


def device_ms(fn, reps):
    for _ in range(2):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def host_ms(fn, reps):
    for _ in range(2):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def lzw_offsets(bits):
    ends = torch.cumsum(bits, dim=1, dtype=torch.int64)
    nbytes = (ends[:, -1].cpu().numpy() + 7) // 8
    starts = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    return (ends - bits + torch.from_numpy(starts * 8).to(DEV)[:, None]).contiguous(), int(nbytes.sum())


def stages(name, host, reps, rows, with_pillow):
    n, H, W, _ = host.shape
    frames = torch.from_numpy(host).to(DEV)
    delays = V.gif_delays(25, n)
    data = V.encode_gif(frames, 25)
    indices, palettes, k = V.quantize_frames(frames)
    im = Image.open(io.BytesIO(data))
    for i in range(n):
        im.seek(i)
        assert np.array_equal(np.asarray(im.convert("RGB")), palettes[0][indices[i].cpu().numpy()]), i
    hist = ops.gif_histogram(frames)
    hist_host = hist.cpu().numpy()
    device_palette = torch.from_numpy(palettes).to(DEV)
    rows_here = V.GIF_STRIP_ROWS
    codes, n_codes, bits = ops.gif_lzw_count(indices, rows_here)
    offsets, total = lzw_offsets(bits)
    out = torch.zeros((total + 3) // 4 * 4, device=DEV, dtype=torch.uint8)
    streams, starts, nbytes = V.gif_code_streams(indices, rows_here)
    pieces = [streams.cpu().numpy()[s:s + b] for s, b in zip(starts, nbytes)]
    rows += [f"### {name}: {n} frames of {H} x {W}, {k} colours, strips of {rows_here} rows; file {len(data)} bytes", "",
             "| stage | clock | ms per clip, median | min | max |", "|---|---|---|---|---|",
             f"| emo_gif_histogram | device events | {stats(device_ms(lambda: ops.gif_histogram(frames), reps))} |",
             f"| the read of the histogram (1 MiB) | host | {stats(host_ms(lambda: hist.cpu(), reps))} |",
             f"| median_cut (numpy) | host | {stats(host_ms(lambda: V.median_cut(hist_host[0]), reps))} |",
             f"| emo_gif_map, {k} entries | device events | {stats(device_ms(lambda: ops.gif_map(frames, device_palette, k), reps))} |",
             f"| emo_gif_lzw_count | device events | {stats(device_ms(lambda: ops.gif_lzw_count(indices, rows_here), reps))} |",
             f"| emo_gif_lzw_emit (into a zeroed buffer; the zeroing is outside) | device events | "
             f"{stats(device_ms(lambda: ops.gif_lzw_emit(codes, n_codes, offsets, out, H, W, rows_here), reps))} |",
             f"| the read of the code streams ({total} bytes) | host | {stats(host_ms(lambda: streams.cpu(), reps))} |",
             f"| gif_container: sub-blocks, tables, extensions | host | {stats(host_ms(lambda: V.gif_container(W, H, palettes, pieces, delays), reps))} |",
             f"| encode_gif, all of the above | host | {stats(host_ms(lambda: V.encode_gif(frames, 25), reps))} |"]
    if with_pillow:
        theirs = pil_gif(host, delays)
        rows.append(f"| frames.cpu() + PIL save(save_all=True) ({len(theirs)} bytes) | host | "
                    f"{stats(host_ms(lambda: pil_gif(frames.cpu().numpy(), delays), max(2, reps // 3)))} |")
    rows.append("")
    return indices


def strip_table(name, indices, reps, rows):
    n, H, W = indices.shape
    rows += [f"### strip_rows on {name}: {n} frames of {H} x {W}", "",
             "| strip_rows | strips per frame | LZW payload, bytes | against one stream | count, ms median (min - max) | emit, ms median (min - max) |",
             "|---|---|---|---|---|---|"]
    whole = None
    results = []
    for s in reversed(STRIPS):
        r = H if s is None else s
        codes, n_codes, bits = ops.gif_lzw_count(indices, r)
        offsets, total = lzw_offsets(bits)
        whole = total if s is None else whole
        out = torch.zeros((total + 3) // 4 * 4, device=DEV, dtype=torch.uint8)
        c = device_ms(lambda: ops.gif_lzw_count(indices, r), reps)
        e = device_ms(lambda: ops.gif_lzw_emit(codes, n_codes, offsets, out, H, W, r), reps)
        results.append(f"| {s} | {-(-H // r)} | {total} | {100.0 * (total - whole) / whole:+.1f} % | {statistics.median(c):.3f} ({min(c):.3f} - {max(c):.3f}) | "
                       f"{statistics.median(e):.3f} ({min(e):.3f} - {max(e):.3f}) |")
    rows += list(reversed(results)) + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this benchmark measures on the GPU only")
    rows = [f"device: {torch.cuda.get_device_name(0)}; {a.reps} repetitions after 2 warm-up runs each; device events around the launches, the host "
            "clock around work that ends on the host", ""]
    kept = {}
    for name, make in (("noisy", noisy), ("portrait", portrait)):
        for n in (12, 48):
            indices = stages(f"{name}, {n} frames", make(n, 512, 512), a.reps, rows, with_pillow=n == 12)
            if n == 12:
                kept[name] = indices
    for name, indices in kept.items():
        strip_table(name, indices, a.reps, rows)
    text = "\n".join(rows)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
