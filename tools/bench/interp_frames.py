"""Times the two stages behind the sampling loop, old path against new, on the device (profiles/interp_frames.md):

  1. frame interpolation at the cfg4 latent shape (1, 4, 48, 64, 64), factor 2: `interpolate_latents` as host-level torch on device
     tensors (about a dozen torch ops and one device-to-host read per generated frame) against emo_interp_frames (two launches), launched
     from Python and replayed from a captured HIP graph;
  2. 8-bit frames at 512 x 512: the float video + device-to-host copy + save_videos_grid's host conversion against the uint8 decode +
     device-to-host copy - for the tail alone (from decoded rows on) and for the whole VAE decode.

Host clock around work that ends in a device synchronise (the old paths end on the host anyway); every variant is warmed up, the two
sides alternate inside each repetition, and the median with the min - max spread over the repetitions is reported.  Outputs are compared
before anything is timed.

    python tools/bench/interp_frames.py [--reps 20] [--frames 4] [--out FILE.md]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from emote_hack_amd import ops as o                      # noqa: E402
from emote_hack_amd import pipeline as P                 # noqa: E402
from emote_hack_amd.synth import seeded_randn, synth_state_dict   # noqa: E402

DEV = "cuda"


def timed_pairs(variants, reps, inner=1):
    """variants: {name: fn}; each repetition runs every variant `inner` times in turn, synchronised -> {name: [ms per run]}"""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) * 1e3 / inner)
    return out


def line(name, ms):
    return f"| {name} | {statistics.median(ms):.3f} | {min(ms):.3f} | {max(ms):.3f} |"


def host_u8(video):
    """save_videos_grid's conversion of a (b, 3, f, H, W) float video on the host: per frame HWC, (x * 255).astype(uint8)"""
    v = video.cpu().numpy()
    return (v.transpose(0, 2, 3, 4, 1) * 255).astype("uint8")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=4, help="frames of the 512 x 512 decode")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this benchmark measures on the GPU only")
    rows = [f"device: {torch.cuda.get_device_name(0)}; {a.reps} repetitions per figure, ms per call: median | min | max", ""]

    # ---- 1. interpolation
    lat = seeded_randn((1, 4, 48, 64, 64), 1).to(DEV)
    stub = object.__new__(P.EMOAnimationPipeline)
    host_slerp = lambda v0, v1, t: P.slerp(v0, v1, t)            # a callable that is not the module's own: the host-level torch path
    old = lambda: stub._interpolate_latents(lat, 2, DEV, host_slerp)
    new = lambda: o.interpolate_frames(lat, 2, "slerp")
    y_old, y_new = old(), new()
    err = float((y_old - y_new).abs().max())
    assert torch.equal(y_old[:, :, ::2], y_new[:, :, ::2]) and err < 1e-5, err
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        new()
        with torch.cuda.graph(g, stream=s):
            y_graph = new()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y_graph, y_new)
    t = timed_pairs({"host-level torch (parent)": old, "emo_interp_frames, launched": new, "emo_interp_frames, graph replay": g.replay}, a.reps)
    rows += ["## interpolate_latents, (1, 4, 48, 64, 64) f32, factor 2, slerp (47 generated frames)", "",
             f"max |old - new| = {err:.3e}; copied frames bit-equal", "", "| path | median | min | max |", "|---|---|---|---|"]
    rows += [line(k, v) for k, v in t.items()] + [""]

    # ---- 2. 8-bit frames at 512 x 512
    from emote_hack_amd.vae import AutoencoderKL, VAE_DEFAULTS, vae_param_shapes
    n, H, W = a.frames, 512, 512
    dec = (seeded_randn((n * H * W, 3), 2) * 0.7).to(DEV).to(torch.bfloat16)
    rows8 = torch.zeros(n * H * W, 8, device=DEV, dtype=torch.bfloat16)
    rows8[:, :3] = dec
    rv = rows8[:, :3]
    tail_old = lambda: host_u8(o.rows_to_video(rv, 1, 3, n, H, W))
    tail_new = lambda: o.rows_to_frames_u8(rv, 1, 3, n, H, W).cpu().numpy()
    assert (tail_old() == tail_new()).all()
    t = timed_pairs({"rows_to_video + D2H (f32) + host uint8": tail_old, "rows_to_frames_u8 + D2H (uint8)": tail_new}, a.reps)
    rows += [f"## decoded rows -> uint8 frames on the host, {n} frames of 512 x 512 (bf16 rows)", "", "| path | median | min | max |", "|---|---|---|---|"]
    rows += [line(k, v) for k, v in t.items()] + [""]

    vae = AutoencoderKL()
    vae.load_state_dict(synth_state_dict(vae_param_shapes(dict(VAE_DEFAULTS)), prefix="vae."))
    vae.to(DEV, torch.bfloat16)
    z = (0.2 * seeded_randn((1, 4, n, 64, 64), 3)).to(DEV)
    full_old = lambda: host_u8(vae.decode_video(z, frames_per_call=n))
    full_new = lambda: vae.decode_video(z, frames_per_call=n, output="uint8").cpu().numpy()
    assert (full_old() == full_new()).all()
    t = timed_pairs({"decode_video + D2H (f32) + host uint8": full_old, "decode_video(output=\"uint8\") + D2H": full_new}, max(a.reps // 4, 3))
    rows += [f"## whole VAE decode to uint8 frames on the host, {n} frames of 512 x 512 (SD VAE shape, synthetic weights, bf16)", "",
             "| path | median | min | max |", "|---|---|---|---|"]
    rows += [line(k, v) for k, v in t.items()] + [""]
    text = "\n".join(rows)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
