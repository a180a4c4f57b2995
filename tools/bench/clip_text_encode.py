#!/usr/bin/env python3
"""Time EMOAnimationPipeline._encode_prompt (EMOAnimationPipeline.py:202-289) on the HIP CLIPTextModel at the SD-1.5 configuration:
a prompt and a negative prompt, max_length padding to 77 -> one encoder call of 2 x 77 ids, 12 layers.  Synthetic name-keyed weights;
a character-level stand-in for CLIPTokenizer (host-side, the same call interface - its cost is part of the figure, like the real
tokenizer's would be).  Median of --iters calls after --warmup, per dtype, each call synchronised.

    timeout -k 10 300 python tools/bench/clip_text_encode.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402


class CharTokenizer:
    model_max_length = 77

    def __call__(self, text, padding="max_length", max_length=None, truncation=False, return_tensors="pt"):
        seqs = [[49406] + [ord(ch) % 256 + 256 for ch in t] + [49407] for t in ([text] if isinstance(text, str) else text)]
        if truncation and max_length is not None:
            seqs = [s[:max_length - 1] + [49407] if len(s) > max_length else s for s in seqs]
        n = max_length if padding == "max_length" else max(len(s) for s in seqs)
        ids = torch.tensor([s + [49407] * (n - len(s)) for s in seqs], dtype=torch.int64)
        return SimpleNamespace(input_ids=ids, attention_mask=torch.ones_like(ids))

    def batch_decode(self, ids):
        return [str(r.tolist()) for r in ids]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emote_hack_amd.clip_text import CLIPTextModel, clip_text_synth_state_dict
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    sd = clip_text_synth_state_dict(device="cuda")          # device draws: 123 M parameters
    pipe = EMOAnimationPipeline.__new__(EMOAnimationPipeline)
    pipe.tokenizer = CharTokenizer()
    res = {"what": "_encode_prompt, SD-1.5 CLIP text encoder, prompt + negative prompt = 2 x 77 ids", "iters": a.iters, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "ms": {}}
    prompt, neg = "a person talking to the camera, high quality", "blurry, low quality"
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        m = CLIPTextModel()
        m.load_state_dict(sd)
        pipe.text_encoder = m.to("cuda", dtype)
        for _ in range(a.warmup):
            pipe._encode_prompt(prompt, "cuda", 1, True, neg)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            e = pipe._encode_prompt(prompt, "cuda", 1, True, neg)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        assert e.shape == (2, 77, 768) and bool(torch.isfinite(e.float()).all())
        res["ms"][str(dtype).replace("torch.", "")] = dict(median=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))
        del pipe.text_encoder, m
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
