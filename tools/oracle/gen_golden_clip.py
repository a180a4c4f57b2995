#!/usr/bin/env python3
"""Generate tests/golden/clip_text.{safetensors,json} from the THIRD-PARTY implementation the reference calls (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/oracle/gen_golden_clip.py

EMOAnimationPipeline._encode_prompt (:202-289) calls transformers' `CLIPTextModel(input_ids)[0]`, the SD-1.5 text encoder
magicanimate/pipelines/animation.py:75-76 loads (no network here, so random-init models of the same class).  This script instantiates
that class from `transformers` (version recorded in the .json), loads name-keyed synthetic weights
(emote_hack_amd.clip_text.clip_text_synth_state_dict - both sides regenerate them, nothing is committed), feeds seeded ids and stores
ONLY inputs and outputs:
  tiny/*   2 layers, 64 wide, 4 heads, 16 positions, B = 2, L = 16; its EOS id (500) is NOT the largest id, so the two pooling
           rules pick different rows: pooler_output (eos_token_id 500: first EOS) and pooler_output_eos2 (argmax of the ids)
  sd15/*   the SD-1.5 configuration, B = 2, L = 77, ids in CLIP's layout (BOS 49406, seeded ids, EOS 49407, padding 49407):
           last_hidden_state, and pooler_output once with eos_token_id = 2 (SD-1.5's legacy config.json: argmax of the ids) and
           once with 49407 (first EOS)
  short/*  the SD-1.5 configuration at L = 12 (padding="longest")
The configurations go into the .json next to the key -> shape list.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

import torch  # noqa: E402
import transformers  # noqa: E402
from safetensors.torch import save_file  # noqa: E402
from transformers import CLIPTextConfig, CLIPTextModel  # noqa: E402

from emote_hack_amd.clip_text import SD15_CONFIG, clip_text_synth_state_dict  # noqa: E402
from tests import cases  # noqa: E402

torch.set_grad_enabled(False)
TINY = dict(vocab_size=1000, hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4, max_position_embeddings=16,
            hidden_act="quick_gelu", layer_norm_eps=1e-5, bos_token_id=499, eos_token_id=500, pad_token_id=1)
BOS, EOS = 49406, 49407


def _text_model(m):
    return getattr(m, "text_model", m)      # transformers < 5 wraps the transformer in `.text_model`; 5.x holds it directly


def full(k):
    return k if k.startswith("text_model.") else "text_model." + k        # the checkpoint spelling on either version


def build(cfg):
    m = CLIPTextModel(CLIPTextConfig(**cfg, attn_implementation="eager")).eval()
    sd = clip_text_synth_state_dict(cfg)
    own = m.state_dict()
    keys = {full(k) for k in own} - {"text_model.embeddings.position_ids"}
    assert keys == set(sd), sorted(keys ^ set(sd))[:5]
    m.load_state_dict({k: sd.get(full(k), own[k]) for k in own}, strict=True)
    return m


def clip_ids(lengths, L, bos, eos, vocab_hi, seed):
    """CLIP's layout: BOS, n seeded word ids, EOS, then EOS as padding (CLIPTokenizer's pad token for SD-1.5)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(lengths), L), eos, dtype=torch.int64)
    for b, n in enumerate(lengths):
        ids[b, 0] = bos
        w = torch.randint(2, vocab_hi, (n,), generator=g)
        ids[b, 1:1 + n] = torch.where((w == bos) | (w == eos), w + 2, w)      # word ids never collide with BOS / EOS
    return ids


def main():
    T = {}
    tiny = build(TINY)
    ids = clip_ids([5, 13], 16, TINY["bos_token_id"], TINY["eos_token_id"], 990, 701)
    o = tiny(ids)
    T["tiny/input_ids"], T["tiny/last_hidden_state"], T["tiny/pooler_output"] = ids, o.last_hidden_state.contiguous(), o.pooler_output.contiguous()
    _text_model(tiny).eos_token_id = 2
    T["tiny/pooler_output_eos2"] = tiny(ids).pooler_output.contiguous()

    sd15 = build(dict(SD15_CONFIG))                           # eos_token_id 2: the legacy file
    ids = clip_ids([9, 31], 77, BOS, EOS, 49400, 702)
    o = sd15(ids)
    T["sd15/input_ids"], T["sd15/last_hidden_state"], T["sd15/pooler_output_eos2"] = ids, o.last_hidden_state.contiguous(), o.pooler_output.contiguous()
    _text_model(sd15).eos_token_id = EOS                        # what CLIPTextTransformer reads from a config with eos_token_id 49407
    T["sd15/pooler_output_eos49407"] = sd15(ids).pooler_output.contiguous()
    _text_model(sd15).eos_token_id = 2
    ids = clip_ids([4, 10], 12, BOS, EOS, 49400, 703)
    o = sd15(ids)
    T["short/input_ids"], T["short/last_hidden_state"], T["short/pooler_output_eos2"] = ids, o.last_hidden_state.contiguous(), o.pooler_output.contiguous()
    save_file(T, os.path.join(cases.GOLDEN_DIR, "clip_text.safetensors"))
    json.dump({"transformers": transformers.__version__, "torch": torch.__version__, "configs": {"tiny": TINY, "sd15": SD15_CONFIG},
               "param_shapes": {full(k): list(v.shape) for k, v in sd15.state_dict().items() if not k.endswith("position_ids")},
               "shapes": {k: list(v.shape) for k, v in T.items()}}, open(os.path.join(cases.GOLDEN_DIR, "clip_text.json"), "w"), indent=1)
    print({k: tuple(v.shape) for k, v in T.items()}, "transformers", transformers.__version__)


if __name__ == "__main__":
    main()
