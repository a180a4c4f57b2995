#!/usr/bin/env python3
"""Generate tests/golden/wav2vec2_large.{safetensors,json} from the THIRD-PARTY implementation the reference calls (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/oracle/gen_golden_wav2vec2_large.py

/root/reference/Net.py:607-648 loads transformers' `Wav2Vec2Model` and reads `.last_hidden_state`; the checkpoints of the
wav2vec2-large family (wav2vec2-large-960h-lv60, large-xlsr-53, XLS-R, large-robust) are that class with three config switches on:
feat_extract_norm "layer", conv_bias, do_stable_layer_norm - and a processor that returns an attention_mask.  Like
gen_golden_wav2vec2.py this script instantiates the class from `transformers` (version recorded in the .json), loads name-keyed synthetic
weights (emote_hack_amd.wav2vec2.wav2vec2_synth_state_dict - both sides regenerate them, nothing is committed), feeds seeded waveforms
(tests/wav2vec2_large_cases.py) and stores ONLY outputs:
  tiny_large/out_<n>        cases.WAV2VEC2_TINY with the three switches on, n = 400 (one frame), 720 (two), 4001 (odd remainders)
  tiny_large/combo_*        the four switch combinations (feat_extract_norm group | layer) x (post-LN | pre-LN), conv biases on, n = 4000
  tiny_large/batch_*        two utterances of 4000 and 2777 samples through the processor (normalised per utterance, right-padded,
                            attention_mask) and the model as ONE batch: the padded input_values, and the valid rows (12 and 8 frames)
  wide/out, out_bf16, out_fp16   LARGE_CONFIG at depth 4 on the 1 s input of the base golden -> (1, 49, 1024): the f32 output and
                            transformers' OWN bf16 / fp16 outputs for the same input (the low-precision yardstick of the GPU tests)
The .json records the versions, the shapes, transformers' key -> shape listing for the tiny and the 24-layer large config, and the
mean / max absolute error of the bf16 / fp16 outputs against the f32 one.
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
from safetensors.torch import load_file, save_file  # noqa: E402
from transformers import Wav2Vec2Config, Wav2Vec2FeatureExtractor, Wav2Vec2Model  # noqa: E402

from emote_hack_amd.wav2vec2 import LARGE_CONFIG, wav2vec2_synth_state_dict  # noqa: E402
from tests import cases  # noqa: E402
from tests import wav2vec2_large_cases as L  # noqa: E402

torch.set_grad_enabled(False)


def build(cfg):
    m = Wav2Vec2Model(Wav2Vec2Config(**cfg)).eval()
    sd = wav2vec2_synth_state_dict(cfg)
    own = m.state_dict()
    assert set(sd) | {"masked_spec_embed"} >= set(own), sorted(set(own) - set(sd))[:5]
    assert set(sd) <= set(own), sorted(set(sd) - set(own))[:5]
    m.load_state_dict({k: sd.get(k, own[k]) for k in own}, strict=True)
    return m


def listing(cfg):
    with torch.device("meta"):
        m = Wav2Vec2Model(Wav2Vec2Config(**cfg))
    return {k: list(v.shape) for k, v in m.state_dict().items()}


def main():
    T, meta = {}, {}
    tiny = build(L.TINY_LARGE)
    for n in L.LENGTHS:
        T[f"tiny_large/out_{n}"] = tiny(L.wave(n)).last_hidden_state.contiguous()
    for norm, stable in L.COMBOS:
        T[L.combo_key(norm, stable)] = build(L.combo_config(norm, stable))(L.wave(L.COMBO_N)).last_hidden_state.contiguous()
    # the padded batch, as the family's processor makes it
    proc = Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True, return_attention_mask=True)
    enc = proc([w.numpy() for w in L.batch_waves()], sampling_rate=16000, padding=True, return_tensors="pt")
    mask = enc.attention_mask
    assert [int(v) for v in mask.sum(1)] == list(L.BATCH_LENGTHS) and mask.shape == (2, max(L.BATCH_LENGTHS))
    hs = tiny(enc.input_values, attention_mask=mask).last_hidden_state
    frames = [int(v) for v in tiny._get_feat_extract_output_lengths(mask.sum(1))]
    assert tuple(frames) == L.BATCH_FRAMES, frames
    T["tiny_large/batch_input_values"] = enc.input_values.contiguous()
    for b, t in enumerate(frames):
        T[f"tiny_large/batch_out_{b}"] = hs[b, :t].contiguous()
        alone = tiny(enc.input_values[b:b + 1, :L.BATCH_LENGTHS[b]]).last_hidden_state[0]        # the equivalence the HIP forward rests on
        meta.setdefault("batch_vs_alone_max_abs", []).append(float((alone - hs[b, :t]).abs().max()))
    # the large widths at depth 4, in f32 and in transformers' own bf16 / fp16
    iv = load_file(os.path.join(cases.GOLDEN_DIR, "wav2vec2.safetensors"))["base/input_values"]
    wide = build(L.WIDE)
    ref = wide(iv).last_hidden_state.contiguous()
    T["wide/out"] = ref
    lowp = {}
    for name, dtype in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        y = wide.to(dtype)(iv.to(dtype)).last_hidden_state.contiguous()
        T[f"wide/out_{name}"] = y
        e = (y.float() - ref).abs()
        lowp[name] = {"mean": float(e.mean()), "max": float(e.max())}
        wide = build(L.WIDE) if name == "bf16" else wide         # fresh f32 weights for the next dtype
    save_file(T, L.GOLDEN)
    meta.update({"transformers": transformers.__version__, "torch": torch.__version__,
                 "shapes": {k: list(v.shape) for k, v in T.items()},
                 "batch": {"lengths": list(L.BATCH_LENGTHS), "frames": frames},
                 "low_precision_error": {"wide": lowp},
                 "state_dict": {"tiny_large": listing(L.TINY_LARGE), "large": listing(LARGE_CONFIG)}})
    json.dump(meta, open(L.GOLDEN_JSON, "w"), indent=1)
    print({k: tuple(v.shape) for k, v in T.items()}, lowp, meta["batch_vs_alone_max_abs"], "transformers", transformers.__version__)


if __name__ == "__main__":
    main()
