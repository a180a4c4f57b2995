"""Times the PNG decoding of a clip's files, stage by stage, beside Pillow on the host (profiles/png_decode.md):

  new   emote_hack_amd.video_io.decode_png: parse_png on the host (chunks, CRCs, the zlib header), one upload of all streams,
        emo_png_inflate, emo_png_unfilter, one small read of the statuses and the rows' Adler-32 pairs, their combination on the host
  old   PIL's `Image.open(f)` + `np.asarray` frame by frame, one host thread, then one `.to(device)` of the stacked frames

at 512 x 512 for 12 frames and for one still, on the two kinds of content of tools/bench/gif.py (`noisy`, `portrait`), for the files of
this project's writer (encode_png: one dynamic block per frame, strips of one row) and for Pillow's (compress_level 6).  The kernels
are timed with device events after a warm-up, the host stages and the whole calls with the host clock around work that ends on the
host; medians with the min - max spread.  Before anything is timed every decoded frame must equal the input.

    python tools/bench/png_decode.py [--reps 10] [--out FILE.md]
"""
import argparse
import io
import os
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from emote_hack_amd import ops                           # noqa: E402
from emote_hack_amd import video_io as V                 # noqa: E402
from gif import device_ms, host_ms, noisy, portrait, stats      # noqa: E402
from png import pil_png                                  # noqa: E402

DEV = "cuda"


def pil_decode(files):
    return torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(f))) for f in files])).to(DEV)


def stages(name, files, host, reps, rows):
    n, H, W, C = host.shape
    assert np.array_equal(V.decode_png(files).cpu().numpy(), host) and np.array_equal(pil_decode(files).cpu().numpy(), host)
    parsed = [V.parse_png(f) for f in files]
    sizes = np.array([len(p.still) for p in parsed], np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    packed = np.concatenate([offsets.view(np.uint8)] + [np.frombuffer(p.still, np.uint8) for p in parsed] + [np.zeros(-int(offsets[-1]) % 4, np.uint8)])
    dev = torch.from_numpy(packed).to(DEV)
    streams, off = dev[8 * (n + 1):], dev[:8 * (n + 1)].view(torch.int64)
    filtered, produced, st1 = ops.png_inflate(streams, off, H, W, C)
    frames, adler, st2 = ops.png_unfilter(filtered, C)
    back = lambda: torch.cat([st1, st2, produced, adler.reshape(-1)]).cpu()
    pairs = adler.cpu().numpy()
    rows += [f"### {name}: {n} frame{'s' if n > 1 else ''} of {H} x {W} x {C}; files {sum(len(f) for f in files)} bytes, deflate streams {int(sizes.sum())} bytes", "",
             "| stage | clock | ms, median | min | max |", "|---|---|---|---|---|",
             f"| parse_png, {n} files (chunks, CRCs) | host | {stats(host_ms(lambda: [V.parse_png(f) for f in files], reps))} |",
             f"| the upload of the streams ({packed.size} bytes) | host | {stats(host_ms(lambda: (torch.from_numpy(packed).to(DEV), torch.cuda.synchronize()), reps))} |",
             f"| emo_png_inflate | device events | {stats(device_ms(lambda: ops.png_inflate(streams, off, H, W, C), reps))} |",
             f"| emo_png_unfilter | device events | {stats(device_ms(lambda: ops.png_unfilter(filtered, C), reps))} |",
             f"| the read of statuses, byte counts and Adler-32 pairs ({(3 * n + adler.numel()) * 4} bytes) | host | {stats(host_ms(back, reps))} |",
             f"| adler32_combine, {n} frames | host | {stats(host_ms(lambda: [V.adler32_combine(a, 1 + W * C) for a in pairs], reps))} |",
             f"| decode_png, all of the above | host | {stats(host_ms(lambda: (V.decode_png(files), torch.cuda.synchronize()), reps))} |",
             f"| PIL Image.open + np.asarray per file, then one .to(device) | host | {stats(host_ms(lambda: (pil_decode(files), torch.cuda.synchronize()), reps))} |",
             ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this benchmark measures on the GPU only")
    rows = [f"device: {torch.cuda.get_device_name(0)}; {a.reps} repetitions after 2 warm-up runs each; device events around the launches, the host "
            "clock around work that ends on the host", ""]
    for name, make in (("noisy", noisy), ("portrait", portrait)):
        host = make(12, 512, 512)
        ours = V.encode_png(torch.from_numpy(host).to(DEV))
        theirs = pil_png(host, 6)
        stages(f"{name}, files of encode_png", ours, host, a.reps, rows)
        stages(f"{name}, files of Pillow (compress_level 6)", theirs, host, a.reps, rows)
        stages(f"{name}, one still of Pillow", theirs[:1], host[:1], a.reps, rows)
    text = "\n".join(rows)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
