#!/usr/bin/env python3
"""Time EMOAnimationPipeline._encode_image on the HIP CLIPVisionModelWithProjection at the ViT-L/14 configuration: one 512 x 512 uint8
frame through CLIPImageProcessor (emo_image_preprocess; tap tables cached after the first call) and the 24-layer tower, B = 1, with
guidance ([zeros, image_embeds]).  Synthetic name-keyed weights.  Median of --iters calls after --warmup, per dtype, each call
synchronised; the launch count of one call comes from a KernelProfiler pass.

    timeout -k 10 300 python tools/bench/clip_vision_encode.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emote_hack_amd import ops
    from emote_hack_amd.clip_vision import CLIPImageProcessor, CLIPVisionModelWithProjection, clip_vision_synth_state_dict
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    sd = clip_vision_synth_state_dict(device="cuda")          # device draws: 304 M parameters
    pipe = EMOAnimationPipeline.__new__(EMOAnimationPipeline)
    pipe.image_processor = CLIPImageProcessor(device="cuda")
    img = torch.randint(0, 256, (512, 512, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    res = {"what": "_encode_image, ViT-L/14 CLIP vision encoder with projection, one 512x512 uint8 frame, B = 1", "iters": a.iters,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "ms": {}, "launches": {}}
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        m = CLIPVisionModelWithProjection()
        m.load_state_dict(sd)
        pipe.image_encoder = m.to("cuda", dtype)
        for _ in range(a.warmup):
            pipe._encode_image(img, "cuda", 1, True)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            e = pipe._encode_image(img, "cuda", 1, True)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        assert e.shape == (2, 1, 768) and bool(torch.isfinite(e.float()).all())
        key = str(dtype).replace("torch.", "")
        res["ms"][key] = dict(median=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))
        # profiled launches (GEMMs, attention, norms, the three new kernels); emo_act is not routed through the profiler: one per layer
        ops.PROFILER = ops.KernelProfiler()
        pipe._encode_image(img, "cuda", 1, True)
        summ = ops.PROFILER.summary()
        ops.PROFILER = None
        res["launches"][key] = {k: v["launches"] for k, v in summ.items()}
        res["launches"][key]["act"] = m.config.num_hidden_layers
        res["launches"][key]["total"] = sum(res["launches"][key].values())
        del pipe.image_encoder, m
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
