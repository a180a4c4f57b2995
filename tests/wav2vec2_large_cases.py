"""Configs and seeded inputs shared by tools/oracle/gen_golden_wav2vec2_large.py and the wav2vec2-large tests: the generator and the
tests regenerate the same name-keyed weights and waveforms, tests/golden/wav2vec2_large.safetensors holds transformers' outputs only."""
import os

from emote_hack_amd.synth import seeded_randn
from emote_hack_amd.wav2vec2 import LARGE_CONFIG
from tests import cases

GOLDEN = os.path.join(cases.GOLDEN_DIR, "wav2vec2_large.safetensors")
GOLDEN_JSON = os.path.join(cases.GOLDEN_DIR, "wav2vec2_large.json")

SWITCHES = dict(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True)
# cases.WAV2VEC2_TINY in the wav2vec2-large layout: a LayerNorm behind every conv, conv biases, pre-LN layers
TINY_LARGE = dict(cases.WAV2VEC2_TINY, **SWITCHES)
# every width LARGE_CONFIG runs (H = 1024, 16 heads of 64, positional groups of 64 channels with K = 8192, intermediate 4096) at depth 4
WIDE = dict(LARGE_CONFIG, num_hidden_layers=4)

# one frame, two frames, an odd remainder at every layer
LENGTHS = (400, 720, 4001)
# the switch combinations transformers accepts, conv biases on: (feat_extract_norm, do_stable_layer_norm)
COMBOS = (("group", False), ("group", True), ("layer", False), ("layer", True))
COMBO_N = 4000
BATCH_LENGTHS = (4000, 2777)
BATCH_FRAMES = (12, 8)


def combo_config(norm, stable):
    return dict(cases.WAV2VEC2_TINY, feat_extract_norm=norm, conv_bias=True, do_stable_layer_norm=stable)


def combo_key(norm, stable):
    return f"tiny_large/combo_{norm}_{'pre' if stable else 'post'}_ln"


def wave(n, seed=601):
    """the (1, n) input of the single-utterance goldens"""
    return 0.5 * seeded_randn((1, n), seed + n)


def batch_waves():
    """the raw utterances of the padded batch, before the processor's normalisation and padding"""
    return [0.3 * seeded_randn((n,), 650 + i) + 0.1 for i, n in enumerate(BATCH_LENGTHS)]
