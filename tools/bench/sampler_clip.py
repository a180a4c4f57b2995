"""Whole cfg2 clips (512^2, 12 frames, bf16, HIP graphs, CFG 7.5, ReferenceNet on) through EMOAnimationPipeline.__call__ per sampler:
DDIM-50, DPM-Solver++ 2M-25, Euler-30, Euler-ancestral-30, LMS-30.  One JSON line per sampler: ms per step and seconds per clip over
the warm calls (the first call - plan + graph capture - is the warm-up), and the SCLK bench.py's ClockSampler saw during them.
Synthetic weights: the lines compare TIME only, not image quality at fewer steps.

    python tools/bench/sampler_clip.py [--calls 2] [--only dpm]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import ClockSampler, build_models  # noqa: E402

SAMPLERS = {   # name -> (class name, steps, ctor kwargs)
    "ddim": ("DDIMScheduler", 50, {}),
    "dpm": ("DPMSolverMultistepScheduler", 25, {}),
    "euler": ("EulerDiscreteScheduler", 30, {}),
    "euler_a": ("EulerAncestralDiscreteScheduler", 30, {}),
    "lms": ("LMSDiscreteScheduler", 30, {}),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2, help="timed clips per sampler after the cold one")
    ap.add_argument("--only", default=None, help="comma-separated subset of " + ",".join(SAMPLERS))
    a = ap.parse_args()
    import emote_hack_amd as E
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    from emote_hack_amd.synth import seeded_randn
    dev, dtype, f_tot = "cuda", torch.bfloat16, 12
    unet, ref = build_models(dev, dtype)
    names = a.only.split(",") if a.only else list(SAMPLERS)
    for name in names:
        cls, steps, skw = SAMPLERS[name]
        sch = getattr(E, cls)(beta_schedule="scaled_linear", **skw)
        pipe = EMOAnimationPipeline(unet=unet, scheduler=sch)
        kw = dict(video_length=f_tot, height=512, width=512, num_inference_steps=steps, guidance_scale=7.5, context_frames=f_tot,
                  context_stride=1, context_overlap=0, output_type="latent", appearance_encoder=ref,
                  text_embeddings=seeded_randn((2, 77, 768), 2), ref_image_latents=seeded_randn((1, 4, 64, 64), 3), seed=0)
        lat0 = seeded_randn((1, 4, f_tot, 64, 64), 1).to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe("", latents=lat0, **kw)
        torch.cuda.synchronize()
        cold = time.perf_counter() - t0
        warm = []
        with ClockSampler() as clk:
            for _ in range(max(1, a.calls)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = pipe("", latents=lat0, **kw).videos
                torch.cuda.synchronize()
                warm.append(time.perf_counter() - t0)
        s = sum(warm) / len(warm)
        print(json.dumps({"sampler": name, "scheduler": cls, "num_inference_steps": steps, "ms_per_step": s / steps * 1e3,
                          "s_per_clip": s, "warm_call_s": warm, "cold_call_s": cold, "clock": clk.summary(),
                          "latents_finite": bool(torch.isfinite(out).all()),
                          "workload": "cfg2 via __call__: 512x512 (64x64 latents), 12 frames, bf16, HIP graphs, CFG 7.5, ReferenceNet"}),
              flush=True)
        pipe.clear_plan_cache()
        del pipe


if __name__ == "__main__":
    main()
