"""Times the decoding of an animated GIF, stage by stage, beside Pillow on the host (profiles/gif_decode.md):

  new   emote_hack_amd.video_io.decode_gif: parse_gif on the host (blocks, sub-blocks joined, the sticky disposal), one upload of all
        frames' LZW data, descriptors and tables, emo_gif_lzw_decode, emo_gif_compose, one small read of the statuses
  old   PIL's `im.seek(k)` + `im.convert("RGB")` frame by frame, one host thread, then one `.to(device)` of the stacked frames

at 512 x 512 for 12 frames and for one still, on the two kinds of content of tools/bench/gif.py (`noisy`, `portrait`), both written by
this project's encode_gif (global table, strips of 8 rows between Clear codes) and, for the 12 frames, by Pillow's `save_all` too
(frames cropped to what changed, one stream per frame).  The kernels are timed with device events after a warm-up, the host stages and
the whole calls with the host clock around work that ends on the host; medians with the min - max spread.  Before anything is timed
every decoded frame must equal what Pillow reads.

    python tools/bench/gif_decode.py [--reps 10] [--out FILE.md]
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

DEV = "cuda"


def pil_decode(data, n):
    im = Image.open(io.BytesIO(data))
    out = []
    for k in range(n):
        im.seek(k)
        out.append(np.asarray(im.convert("RGB")))
    return torch.from_numpy(np.stack(out)).to(DEV)


def stages(name, data, n, reps, rows):
    want = pil_decode(data, n).cpu().numpy()
    assert np.array_equal(V.decode_gif(data, select=slice(0, n))[0].cpu().numpy(), want)
    p = V.parse_gif(data)
    fr = p.frames[:n]
    offsets = np.concatenate([[0], np.cumsum([len(f.data) for f in fr])]).astype(np.int64)
    out_offsets = np.concatenate([[0], np.cumsum([f.width * f.height for f in fr])]).astype(np.int64)
    code = np.array([f.code_size for f in fr], np.int32)
    pad = -int(offsets[-1]) % 4
    packed = np.concatenate([np.frombuffer(f.data, np.uint8) for f in fr] + [np.zeros(pad, np.uint8)])
    streams, d_off, d_out, d_code = (torch.from_numpy(a).to(DEV) for a in (packed, offsets, out_offsets, code))
    d_desc = torch.from_numpy(V.gif_descriptors(fr, {k: k for k in range(n)})).to(DEV)
    d_tables = torch.from_numpy(p.tables).to(DEV)
    total = int(out_offsets[-1])
    indices, produced, st1 = ops.gif_lzw_decode(streams, d_off, d_code, d_out, total)
    rgb, st2 = ops.gif_compose(indices, d_out, d_desc, d_tables, n, p.height, p.width)
    assert np.array_equal(rgb.cpu().numpy(), want)
    upload = packed.size + 16 * (n + 1) + 4 * n + d_desc.numel() * 4 + d_tables.numel()
    rows += [f"### {name}: {n} frame{'s' if n > 1 else ''} on a screen of {p.height} x {p.width}; file {len(data)} bytes, LZW data {int(offsets[-1])} bytes, "
             f"{total} colour indices", "",
             "| stage | clock | ms, median | min | max |", "|---|---|---|---|---|",
             f"| parse_gif (blocks, sub-blocks joined) | host | {stats(host_ms(lambda: V.parse_gif(data), reps))} |",
             f"| the upload of streams, descriptors and tables ({upload} bytes) | host | {stats(host_ms(lambda: (torch.from_numpy(packed).to(DEV), torch.cuda.synchronize()), reps))} |",
             f"| emo_gif_lzw_decode | device events | {stats(device_ms(lambda: ops.gif_lzw_decode(streams, d_off, d_code, d_out, total), reps))} |",
             f"| emo_gif_compose | device events | {stats(device_ms(lambda: ops.gif_compose(indices, d_out, d_desc, d_tables, n, p.height, p.width), reps))} |",
             f"| the read of statuses and counts ({12 * n} bytes) | host | {stats(host_ms(lambda: torch.cat([st1, st2, produced]).cpu(), reps))} |",
             f"| decode_gif, all of the above | host | {stats(host_ms(lambda: (V.decode_gif(data, select=slice(0, n)), torch.cuda.synchronize()), reps))} |",
             f"| PIL seek + convert(\"RGB\") per frame, then one .to(device) | host | {stats(host_ms(lambda: (pil_decode(data, n), torch.cuda.synchronize()), reps))} |",
             ""]


def pil_gif(host):
    frames = [Image.fromarray(f, "RGB") for f in host]
    buf = io.BytesIO()
    frames[0].save(buf, "GIF", save_all=True, append_images=frames[1:], duration=40, loop=0)
    return buf.getvalue()


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
        ours = V.encode_gif(torch.from_numpy(host).to(DEV), 25)
        stages(f"{name}, file of encode_gif", ours, 12, a.reps, rows)
        stages(f"{name}, file of Pillow (save_all)", pil_gif(host), 12, a.reps, rows)
        stages(f"{name}, the first frame of encode_gif's file alone", ours, 1, a.reps, rows)
    text = "\n".join(rows)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
