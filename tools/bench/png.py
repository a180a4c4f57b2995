"""Times the PNG encoding of a clip's 8-bit frames, stage by stage, beside Pillow on the host (profiles/png_encode.md):

  new   emote_hack_amd.video_io.encode_png: emo_png_filter, emo_png_lz_count, the read of the histograms and the Adler-32 pairs, the
        Huffman tables and block headers on the host, emo_png_deflate_bits, emo_png_deflate_emit, one device-to-host copy of the
        streams, the header / end-of-block / checksum and the chunks on the host
  old   a device-to-host copy of the uint8 frames, then PIL's `save(format="PNG")` frame by frame at compress_level 6 (its default) and
        1, one host thread

at 512 x 512, the size the pipeline is benchmarked at, for 12 and for 48 frames, on the two kinds of content of tools/bench/gif.py:
`noisy` (waves, ramps, N(0, 6) noise) and `portrait` (a flat background behind a textured, moving oval).  The kernels are timed with
device events after a warm-up, the host stages and the whole calls with the host clock around work that ends on the host; medians with
the min - max spread.  A second table gives the file size and the kernels' times for strip_rows in 1, 2, 4, 8, 16, 32 and None (the largest
strip that fits 65535 bytes).  Before anything is timed, Pillow decodes the device's files and every frame must equal the input.

    python tools/bench/png.py [--reps 10] [--out FILE.md]
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
from emote_hack_amd import ops                           # noqa: E402
from emote_hack_amd import video_io as V                 # noqa: E402
from gif import device_ms, host_ms, noisy, portrait, stats      # noqa: E402

DEV = "cuda"
STRIPS = (1, 2, 4, 8, 16, 32, None)


def pil_png(host, level):
    out = []
    for f in host:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, format="PNG", compress_level=level)
        out.append(buf.getvalue())
    return out


def prepared(frames, strip_rows):
    """the intermediate buffers of png_zlib_streams, so that every stage can be timed on its own"""
    n, H, W, C = frames.shape
    rows = V.png_strip_rows(strip_rows, H, W, C)
    filtered, adler = ops.png_filter(frames, 5)
    tokens, n_tokens, hist = ops.png_lz_count(filtered, C, rows)
    hist_host = hist.cpu().numpy()
    tables = [V.deflate_tables(h) for h in hist_host]
    codes = torch.from_numpy(np.stack([t.codes for t in tables]).view(np.int32)).to(DEV)
    bits = ops.png_deflate_bits(tokens, n_tokens, codes, H, W, C, rows)
    token_bits = np.array([t.token_bits(h) for t, h in zip(tables, hist_host)], np.int64)
    head = np.array([16 + t.header_bits for t in tables], np.int64)
    nbytes = (head + token_bits + np.array([t.end_of_block[1] for t in tables], np.int64) + 7) // 8 + 4
    starts = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    ends = torch.cumsum(bits, dim=1, dtype=torch.int64)
    offsets = (ends - bits + torch.from_numpy(starts * 8 + head).to(DEV)[:, None]).contiguous()
    out = torch.zeros((int(nbytes.sum()) + 3) // 4 * 4, device=DEV, dtype=torch.uint8)
    ops.png_deflate_emit(tokens, n_tokens, codes, offsets, out, H, W, C, rows)
    return dict(rows=rows, filtered=filtered, adler=adler, tokens=tokens, n_tokens=n_tokens, hist=hist, hist_host=hist_host, tables=tables,
                codes=codes, bits=bits, token_bits=token_bits, starts=starts, nbytes=nbytes, offsets=offsets, out=out)


def stages(name, host, reps, rows, with_pillow):
    n, H, W, C = host.shape
    frames = torch.from_numpy(host).to(DEV)
    files = V.encode_png(frames)
    for i in range(n):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[i]))), host[i]), i
    p = prepared(frames, V.PNG_STRIP_ROWS)
    r = p["rows"]
    out_host, adler_host = p["out"].cpu().numpy(), p["adler"].cpu().numpy()
    size = sum(len(f) for f in files)

    def finish():
        return [V.png_container(W, H, C, V.zlib_stream(out_host[s:s + b], t, tb, V.adler32_combine(a, 1 + W * C)))
                for s, b, t, tb, a in zip(p["starts"], p["nbytes"], p["tables"], p["token_bits"], adler_host)]

    rows += [f"### {name}: {n} frames of {H} x {W} x {C}, adaptive filter, strips of {r} rows; files {size} bytes, {size / host.size:.4f} of the raw frames", "",
             "| stage | clock | ms per clip, median | min | max |", "|---|---|---|---|---|",
             f"| emo_png_filter | device events | {stats(device_ms(lambda: ops.png_filter(frames, 5), reps))} |",
             f"| emo_png_lz_count | device events | {stats(device_ms(lambda: ops.png_lz_count(p['filtered'], C, r), reps))} |",
             f"| the read of the histograms and Adler-32 pairs ({p['hist'].numel() * 4 + p['adler'].numel() * 4} bytes) | host | "
             f"{stats(host_ms(lambda: (p['hist'].cpu(), p['adler'].cpu()), reps))} |",
             f"| deflate_tables, {n} frames (Python) | host | {stats(host_ms(lambda: [V.deflate_tables(h) for h in p['hist_host']], reps))} |",
             f"| emo_png_deflate_bits | device events | "
             f"{stats(device_ms(lambda: ops.png_deflate_bits(p['tokens'], p['n_tokens'], p['codes'], H, W, C, r), reps))} |",
             f"| emo_png_deflate_emit (into a zeroed buffer; the zeroing is outside) | device events | "
             f"{stats(device_ms(lambda: ops.png_deflate_emit(p['tokens'], p['n_tokens'], p['codes'], p['offsets'], p['out'], H, W, C, r), reps))} |",
             f"| the read of the streams ({p['out'].numel()} bytes) | host | {stats(host_ms(lambda: p['out'].cpu(), reps))} |",
             f"| header, end-of-block, Adler-32, chunks and CRCs | host | {stats(host_ms(finish, reps))} |",
             f"| encode_png, all of the above | host | {stats(host_ms(lambda: V.encode_png(frames), reps))} |"]
    if with_pillow:
        for level in (6, 1):
            theirs = sum(len(f) for f in pil_png(host, level))
            rows.append(f"| frames.cpu() + PIL save(format=\"PNG\", compress_level={level}) ({theirs} bytes; ours {100.0 * (size - theirs) / theirs:+.1f} %) | host | "
                        f"{stats(host_ms(lambda: pil_png(frames.cpu().numpy(), level), max(2, reps // 3)))} |")
    rows.append("")
    return frames


def strip_table(name, frames, reps, rows):
    n, H, W, C = frames.shape
    rows += [f"### strip_rows on {name}: {n} frames of {H} x {W} x {C}", "",
             "| strip_rows | rows per strip | strips per frame | files, bytes | against strips of 8 | lz_count, ms median (min - max) | "
             "deflate_bits + deflate_emit, ms median (min - max) | encode_png, ms median (min - max) |", "|---|---|---|---|---|---|---|---|"]
    base = sum(len(f) for f in V.encode_png(frames, strip_rows=8))
    for s in STRIPS:
        p = prepared(frames, s)
        r = p["rows"]
        size = sum(len(f) for f in V.encode_png(frames, strip_rows=s))
        c = device_ms(lambda: ops.png_lz_count(p["filtered"], C, r), reps)
        e = device_ms(lambda: (ops.png_deflate_bits(p["tokens"], p["n_tokens"], p["codes"], H, W, C, r),
                               ops.png_deflate_emit(p["tokens"], p["n_tokens"], p["codes"], p["offsets"], p["out"], H, W, C, r)), reps)
        w = host_ms(lambda: V.encode_png(frames, strip_rows=s), reps)
        rows.append(f"| {s} | {r} | {-(-H // r)} | {size} | {100.0 * (size - base) / base:+.2f} % | {statistics.median(c):.3f} ({min(c):.3f} - {max(c):.3f}) | "
                    f"{statistics.median(e):.3f} ({min(e):.3f} - {max(e):.3f}) | {statistics.median(w):.3f} ({min(w):.3f} - {max(w):.3f}) |")
    rows.append("")


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
            frames = stages(f"{name}, {n} frames", make(n, 512, 512), a.reps, rows, with_pillow=n == 12)
            if n == 12:
                kept[name] = frames
    for name, frames in kept.items():
        strip_table(name, frames, a.reps, rows)
    text = "\n".join(rows)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
