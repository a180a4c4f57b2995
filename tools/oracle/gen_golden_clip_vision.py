#!/usr/bin/env python3
"""Generate tests/golden/clip_vision.{safetensors,json} from the THIRD-PARTY implementation the reference calls (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/oracle/gen_golden_clip_vision.py

EMOAnimationPipeline.py:867 loads transformers' `CLIPVisionModelWithProjection` as the pipeline's `image_encoder` (:909-917), and
videonet_animatediff.py:9 imports `CLIPImageProcessor` next to it (no network here, so random-init models of the same class).  This
script instantiates both classes from `transformers` (versions recorded in the .json), loads name-keyed synthetic weights
(emote_hack_amd.clip_vision.clip_vision_synth_state_dict - both sides regenerate them, nothing is committed) and stores ONLY outputs:
  tiny/*    2 layers, 64 wide, 4 heads, image 42, patch 14 (10 tokens, the K = 588 pad), projection 32, B = 2: last_hidden_state,
            pooler_output, image_embeds and every hidden state in full
  vitl14/*  the ViT-L/14 default configuration, B = 2: image_embeds, pooler_output, every 8th token row (row 0 included) of
            last_hidden_state and of hidden_states[-2]
  pixel_values are regenerated from a seed on both sides (model_pixels), never stored.
  proc/<H>x<W>  every 4th row / column of the pixel_values transformers' own PIL-backed CLIPImageProcessor returns for a seeded smooth
            uint8 image (smooth_image: low-frequency pattern plus mild noise) - 512x512, 480x640, 768x512, 300x200, 224x224
The .json holds the versions, the configurations, the key -> shape listing of CLIPVisionModelWithProjection, per processor image the max
and mean difference between the CPU f32 definition (definition_pixels) and that PIL output, and the error of transformers' own model
run in bf16 / fp16 on the CPU against its f32 output (the low-precision yardstick of tests/test_gpu_clip_vision.py).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import PIL  # noqa: E402
import torch  # noqa: E402
import transformers  # noqa: E402
from PIL import Image  # noqa: E402
from safetensors.torch import save_file  # noqa: E402
from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection  # noqa: E402

from emote_hack_amd.clip_vision import (OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, VITL14_CONFIG, center_crop_offsets,  # noqa: E402
                                        clip_vision_synth_state_dict, resize_output_size)
from emote_hack_amd.synth import seeded_randn  # noqa: E402
from tests import cases  # noqa: E402

torch.set_grad_enabled(False)
TINY = dict(hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4, num_channels=3, image_size=42, patch_size=14,
            projection_dim=32, hidden_act="quick_gelu", layer_norm_eps=1e-5)
PROC_SIZES = [(512, 512), (480, 640), (768, 512), (300, 200), (224, 224)]      # (H, W)
PIXEL_SEED = {"tiny": 801, "vitl14": 802}
PROC_SEED = 810


def model_pixels(name, cfg, batch=2):
    """The model cases' input: N(0, 1) `pixel_values` (about the range of normalised images), from a seed."""
    return seeded_randn((batch, 3, cfg["image_size"], cfg["image_size"]), PIXEL_SEED[name])


def smooth_image(H, W, seed):
    """A smooth uint8 RGB test image: per channel a sum of three low-frequency 2-D cosines with seeded frequencies (<= 3 periods over
    the image), phases and amplitudes around mid-grey, plus uniform noise of +-6 levels; rounded and clipped to [0, 255]."""
    g = torch.Generator().manual_seed(seed)
    yy = torch.arange(H, dtype=torch.float64)[:, None] / H
    xx = torch.arange(W, dtype=torch.float64)[None, :] / W
    img = torch.empty(H, W, 3, dtype=torch.float64)
    for c in range(3):
        fr = torch.rand(3, 2, generator=g, dtype=torch.float64) * 3.0
        ph = torch.rand(3, generator=g, dtype=torch.float64) * 6.283185307179586
        am = 20.0 + torch.rand(3, generator=g, dtype=torch.float64) * 25.0
        v = torch.full((H, W), 128.0, dtype=torch.float64)
        for k in range(3):
            v = v + am[k] * torch.cos(6.283185307179586 * (fr[k, 0] * yy + fr[k, 1] * xx) + ph[k])
        img[:, :, c] = v
    img = img + (torch.rand(H, W, 3, generator=g, dtype=torch.float64) * 12.0 - 6.0)
    return img.round().clamp(0, 255).to(torch.uint8)


def definition_pixels(img_u8, shortest_edge=224, crop=224):
    """The arithmetic definition of emo_image_preprocess on the CPU, f32: antialiased bicubic interpolate to transformers' shortest-edge
    size, centre crop, clamp, * 1/255, normalise - no rounding to uint8 in between."""
    H, W, _ = img_u8.shape
    rh, rw = resize_output_size(H, W, shortest_edge)
    top, left = center_crop_offsets(rh, rw, crop)
    x = img_u8.permute(2, 0, 1)[None].float()
    y = torch.nn.functional.interpolate(x, size=(rh, rw), mode="bicubic", antialias=True, align_corners=False)
    y = y[0, :, top:top + crop, left:left + crop].clamp(0, 255) * (1.0 / 255.0)
    return (y - torch.tensor(OPENAI_CLIP_MEAN)[:, None, None]) / torch.tensor(OPENAI_CLIP_STD)[:, None, None]


def full(k):
    return k if k.startswith(("vision_model.", "visual_projection.")) else "vision_model." + k


def build(cfg, dtype=torch.float32):
    m = CLIPVisionModelWithProjection(CLIPVisionConfig(**cfg, attn_implementation="eager")).eval()
    sd = clip_vision_synth_state_dict(cfg)
    own = m.state_dict()
    keys = {full(k) for k in own} - {"vision_model.embeddings.position_ids"}
    assert keys == set(sd), sorted(keys ^ set(sd))[:5]
    m.load_state_dict({k: sd.get(full(k), own[k]) for k in own}, strict=True)
    return m.to(dtype)


def lowp_error(cfg, name, ref):
    """transformers' own model in bf16 / fp16 on the CPU (weights and pixel_values rounded to the dtype) against its f32 output"""
    out = {}
    for dt, tag in ((torch.bfloat16, "bfloat16"), (torch.float16, "float16")):
        o = build(cfg, dt)(model_pixels(name, cfg).to(dt), output_hidden_states=False)
        out[tag] = {}
        for k in ("last_hidden_state", "image_embeds"):
            e = (getattr(o, k).float() - getattr(ref, k)).abs()
            out[tag][k] = {"mean": float(e.mean()), "max": float(e.max())}
    return out


def main():
    T, meta = {}, {}
    tiny = build(TINY)
    o = tiny(model_pixels("tiny", TINY), output_hidden_states=True)
    assert len(o.hidden_states) == TINY["num_hidden_layers"] + 1 and torch.equal(o.hidden_states[-1], o.last_hidden_state)
    T["tiny/last_hidden_state"], T["tiny/pooler_output"], T["tiny/image_embeds"] = o.last_hidden_state, tiny_pool(tiny, o), o.image_embeds
    for i, h in enumerate(o.hidden_states):
        T[f"tiny/hidden_states.{i}"] = h
    lowp = {"tiny": lowp_error(TINY, "tiny", o)}

    big = build(dict(VITL14_CONFIG))
    o = big(model_pixels("vitl14", VITL14_CONFIG), output_hidden_states=True)
    T["vitl14/image_embeds"], T["vitl14/pooler_output"] = o.image_embeds, tiny_pool(big, o)
    T["vitl14/last_hidden_state_rows8"] = o.last_hidden_state[:, ::8]
    T["vitl14/hidden_states_m2_rows8"] = o.hidden_states[-2][:, ::8]
    lowp["vitl14"] = lowp_error(VITL14_CONFIG, "vitl14", o)
    param_shapes = {full(k): list(v.shape) for k, v in big.state_dict().items() if not k.endswith("position_ids")}

    with_tv = getattr(transformers, "CLIPImageProcessorPil", None)         # the PIL-backed class under either transformers generation
    proc = (with_tv or transformers.CLIPImageProcessor)()
    meta["processor_class"] = type(proc).__name__
    pstats = {}
    for i, (H, W) in enumerate(PROC_SIZES):
        img = smooth_image(H, W, PROC_SEED + i)
        pil = torch.as_tensor(np.asarray(proc(Image.fromarray(img.numpy()), return_tensors="pt").pixel_values))[0].float()
        assert tuple(pil.shape) == (3, 224, 224), pil.shape
        d = (definition_pixels(img) - pil).abs()
        pstats[f"{H}x{W}"] = {"max": float(d.max()), "mean": float(d.mean()), "resized": list(resize_output_size(H, W, 224)),
                              "crop_top_left": list(center_crop_offsets(*resize_output_size(H, W, 224), 224))}
        T[f"proc/{H}x{W}"] = pil[:, ::4, ::4]
    T = {k: v.contiguous().clone() for k, v in T.items()}
    save_file(T, os.path.join(cases.GOLDEN_DIR, "clip_vision.safetensors"))
    json.dump({"transformers": transformers.__version__, "torch": torch.__version__, "PIL": PIL.__version__, **meta,
               "configs": {"tiny": TINY, "vitl14": VITL14_CONFIG}, "pixel_seed": PIXEL_SEED, "proc_seed": PROC_SEED,
               "param_shapes": param_shapes, "processor_definition_vs_pil": pstats, "low_precision_error": lowp,
               "shapes": {k: list(v.shape) for k, v in T.items()}}, open(os.path.join(cases.GOLDEN_DIR, "clip_vision.json"), "w"), indent=1)
    print({k: tuple(v.shape) for k, v in T.items()}, "transformers", transformers.__version__)
    print(json.dumps(pstats), json.dumps(lowp))


def tiny_pool(m, o):
    """pooler_output: the with-projection output of some transformers versions does not carry it - post_layernorm of the class token"""
    p = getattr(o, "pooler_output", None)
    if p is not None:
        return p
    vm = getattr(m, "vision_model", m)
    return vm.post_layernorm(o.last_hidden_state[:, 0])


if __name__ == "__main__":
    main()
