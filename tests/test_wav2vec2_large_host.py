"""Host-side checks (no GPU) of the wav2vec2-large family: the key listing against transformers' own state dict (recorded in
tests/golden/wav2vec2_large.json), the constructor's switches, attention_mask validation, from_pretrained on a local folder, and the
argument checks of emo_layernorm_act / emo_wav_conv0_ln_act through ctypes (their pointers are never dereferenced on the host)."""
import ctypes as C
import json

import pytest
import torch

from tests import cases
from tests import wav2vec2_large_cases as L

BAD_SHAPE, BAD_DTYPE, UNSUPPORTED, NULL = -1, -2, -3, -5


@pytest.fixture(scope="module")
def meta():
    with open(L.GOLDEN_JSON) as f:
        return json.load(f)


def _listing(meta, name):
    return {k: tuple(v) for k, v in meta["state_dict"][name].items() if k != "masked_spec_embed"}


def test_param_shapes_equal_transformers_listing(meta):
    from emote_hack_amd.wav2vec2 import LARGE_CONFIG, wav2vec2_param_shapes
    for name, cfg in (("tiny_large", L.TINY_LARGE), ("large", LARGE_CONFIG)):
        own = {k: tuple(v) for k, v in wav2vec2_param_shapes(cfg).items()}
        assert own == _listing(meta, name), (name, set(own) ^ set(_listing(meta, name)))
    assert LARGE_CONFIG["hidden_size"] == 1024 and LARGE_CONFIG["num_hidden_layers"] == 24 and LARGE_CONFIG["num_attention_heads"] == 16
    assert LARGE_CONFIG["intermediate_size"] == 4096 and all(LARGE_CONFIG[k] == v for k, v in L.SWITCHES.items())


def test_base_family_listing_and_synthetic_values_are_unchanged():
    """the base family's keys have no conv bias and one norm behind layer 0; the name-keyed generator gives a key the same values
    whichever config lists it"""
    from emote_hack_amd.synth import synth_tensor
    from emote_hack_amd.wav2vec2 import wav2vec2_param_shapes, wav2vec2_synth_state_dict
    base = wav2vec2_param_shapes(cases.WAV2VEC2_TINY)
    fe = sorted(k for k in base if k.startswith("feature_extractor."))
    assert fe == sorted([f"feature_extractor.conv_layers.{i}.conv.weight" for i in range(7)] +
                        ["feature_extractor.conv_layers.0.layer_norm.weight", "feature_extractor.conv_layers.0.layer_norm.bias"])
    assert len(base) == 9 + 4 + 5 + 2 * 16
    large = wav2vec2_param_shapes(L.TINY_LARGE)
    assert set(base) < set(large) and len(large) - len(base) == 7 + 2 * 6
    sb, sl = wav2vec2_synth_state_dict(cases.WAV2VEC2_TINY), wav2vec2_synth_state_dict(L.TINY_LARGE)
    for k in base:
        assert torch.equal(sb[k], sl[k]), k
    k = "feature_projection.projection.weight"
    assert torch.equal(sb[k], synth_tensor("wav2vec2." + k, base[k]))


@pytest.mark.parametrize("norm", ["group", "layer"])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("stable", [False, True])
def test_constructor_accepts_the_switches(norm, bias, stable):
    from emote_hack_amd.wav2vec2 import Wav2Vec2Model, wav2vec2_param_shapes, wav2vec2_synth_state_dict
    cfg = dict(cases.WAV2VEC2_TINY, feat_extract_norm=norm, conv_bias=bias, do_stable_layer_norm=stable)
    m = Wav2Vec2Model(cfg)
    assert (m.config.feat_extract_norm, m.config.conv_bias, m.config.do_stable_layer_norm) == (norm, bias, stable)
    missing, unexpected = m.load_state_dict(wav2vec2_synth_state_dict(cfg))
    assert not missing and not unexpected and set(m.state_dict()) == set(wav2vec2_param_shapes(cfg))
    assert m.conv0_route in m.CONV0_ROUTES


def test_constructor_builds_the_large_config_and_refuses_an_unknown_norm():
    from emote_hack_amd.wav2vec2 import LARGE_CONFIG, Wav2Vec2Model
    m = Wav2Vec2Model(LARGE_CONFIG)
    assert m.config.hidden_size == 1024 and len(m._shapes) == 7 * 4 + 4 + 5 + 24 * 16
    with pytest.raises(ValueError, match="feat_extract_norm"):
        Wav2Vec2Model(dict(cases.WAV2VEC2_TINY, feat_extract_norm="batch"))


def test_mask_validation_runs_before_any_device_work():
    """refusals come from the arguments alone: the models here hold no weights and sit on the CPU"""
    from emote_hack_amd._lib import EmoHipError
    from emote_hack_amd.wav2vec2 import Wav2Vec2Model
    m = Wav2Vec2Model(L.TINY_LARGE)
    x = torch.zeros(2, 4000)
    ok = torch.ones(2, 4000, dtype=torch.long)
    ok[1, 2777:] = 0
    holes = ok.clone()
    holes[1, 100] = 0
    with pytest.raises(ValueError, match="right-padded"):
        m(x, attention_mask=holes)
    left = torch.ones(2, 4000, dtype=torch.long)
    left[1, :50] = 0
    with pytest.raises(ValueError, match="right-padded"):
        m(x, attention_mask=left)
    with pytest.raises(ValueError, match="shape"):
        m(x, attention_mask=ok[:, :3999])
    with pytest.raises(ValueError, match="shape"):
        m(x, attention_mask=ok[:1])
    with pytest.raises(ValueError, match="0 / 1"):
        m(x, attention_mask=ok * 2)
    short = ok.clone()
    short[1, 300:] = 0          # 300 samples: the feature encoder runs dry
    with pytest.raises(ValueError, match="too short"):
        m(x, attention_mask=short)
    with pytest.raises(ValueError, match="conv0_route"):
        m(x, attention_mask=ok, conv0_route="im2col")
    with pytest.raises(EmoHipError):            # a valid call gets as far as the missing weights
        m(x, attention_mask=ok)
    g = Wav2Vec2Model(cases.WAV2VEC2_TINY)
    with pytest.raises(NotImplementedError, match="attention_mask"):
        g(x[:1], attention_mask=ok[:1])
    with pytest.raises(NotImplementedError, match="attention_mask"):
        Wav2Vec2Model(dict(cases.WAV2VEC2_TINY, conv_bias=True, do_stable_layer_norm=True))(x[:1], attention_mask=torch.ones(1, 4000))
    with pytest.raises(ValueError, match="one utterance"):
        g(x)


def test_from_pretrained_reads_a_local_ctc_folder(tmp_path):
    from safetensors.torch import save_file
    from emote_hack_amd.wav2vec2 import Wav2Vec2Model, wav2vec2_synth_state_dict
    sd = wav2vec2_synth_state_dict(L.TINY_LARGE)
    ctc = {"wav2vec2." + k: v for k, v in sd.items()}
    ctc.update({"wav2vec2.masked_spec_embed": torch.zeros(64), "lm_head.weight": torch.zeros(32, 64), "lm_head.bias": torch.zeros(32),
                "quantizer.codevectors": torch.zeros(1, 8, 4), "project_hid.weight": torch.zeros(8, 64), "project_q.bias": torch.zeros(8)})
    folder = tmp_path / "xlsr" / "audio_encoder"
    folder.mkdir(parents=True)
    save_file(ctc, str(folder / "model.safetensors"))
    config = dict(L.TINY_LARGE, conv_dim=list(L.TINY_LARGE["conv_dim"]), model_type="wav2vec2", architectures=["Wav2Vec2ForCTC"], vocab_size=32)
    (folder / "config.json").write_text(json.dumps(config))
    for args in ((str(folder),), (str(tmp_path / "xlsr"), "audio_encoder")):
        m = Wav2Vec2Model.from_pretrained(*args, torch_dtype=torch.bfloat16)
        assert (m.config.feat_extract_norm, m.config.conv_bias, m.config.do_stable_layer_norm) == ("layer", True, True)
        assert m.dtype == torch.bfloat16 and m.config.hidden_size == 64
        got = m.state_dict()
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    # a bare Wav2Vec2Model file (no prefix) of the base family loads through the same door
    base = tmp_path / "base"
    base.mkdir()
    save_file(wav2vec2_synth_state_dict(cases.WAV2VEC2_TINY), str(base / "model.safetensors"))
    (base / "config.json").write_text(json.dumps(dict(cases.WAV2VEC2_TINY, conv_dim=[32] * 7)))
    assert Wav2Vec2Model.from_pretrained(str(base)).config.feat_extract_norm == "group"
    # a key that belongs to no tolerated head is still an error, and so is a missing config.json - by its path
    save_file(dict(ctc, **{"classifier.weight": torch.zeros(2, 64)}), str(folder / "model.safetensors"))
    with pytest.raises(RuntimeError, match="unexpected"):
        Wav2Vec2Model.from_pretrained(str(folder))
    with pytest.raises(RuntimeError, match="config.json"):
        Wav2Vec2Model.from_pretrained(str(tmp_path / "nowhere"))


def test_layernorm_act_argument_checks_run_before_any_launch():
    from emote_hack_amd import _lib
    lib = _lib.load()
    fake = 0x1000

    def call(x=fake, ldx=512, g=fake, b=fake, y=fake, ldy=512, M=64, Cc=512, act=1, dtype=_lib.EMO_BF16):
        return lib.emo_layernorm_act(x, ldx, g, b, y, ldy, M, Cc, 1e-5, act, dtype, None)

    for kw in (dict(x=None), dict(g=None), dict(b=None), dict(y=None)):
        assert call(**kw) == NULL and b"emo_layernorm_act: null" in lib.emo_last_error_string()
    assert call(dtype=7) == BAD_DTYPE
    for kw in (dict(M=0), dict(Cc=508), dict(ldx=504), dict(ldy=500), dict(dtype=_lib.EMO_F32, Cc=510), dict(act=2), dict(g=fake + 4)):
        assert call(**kw) == BAD_SHAPE, kw
    assert call(Cc=2568, ldx=2568, ldy=2568) == UNSUPPORTED and b"too wide" in lib.emo_last_error_string()     # emo_layernorm's limit
    # emo_layernorm_plan describes its launch: the same refusals, the same geometry for both entries
    plan = (C.c_int * 4)(-1, -1, -1, -1)
    assert lib.emo_layernorm_plan(64, 2568, _lib.EMO_BF16, plan) == UNSUPPORTED and list(plan) == [-1] * 4
    assert lib.emo_layernorm_plan(3199, 512, _lib.EMO_BF16, plan) == 0 and list(plan) == [16, 4, 200, 0]


def test_wav_conv0_ln_act_argument_checks_run_before_any_launch():
    from emote_hack_amd import _lib, ops
    lib = _lib.load()
    fake = 0x1000

    def call(wave=fake, n=16000, w=fake, bias=fake, g=fake, b=fake, y=fake, ldy=None, Cc=512, k=10, stride=5, act=1, dtype=_lib.EMO_BF16):
        return lib.emo_wav_conv0_ln_act(wave, n, w, bias, g, b, y, Cc if ldy is None else ldy, Cc, k, stride, 1e-5, act, dtype, None)

    for kw in (dict(wave=None), dict(w=None), dict(bias=None), dict(g=None), dict(b=None), dict(y=None)):
        assert call(**kw) == NULL and b"emo_wav_conv0_ln_act: null" in lib.emo_last_error_string()
    assert call(dtype=5) == BAD_DTYPE
    refused = (dict(Cc=36), dict(Cc=1032), dict(Cc=0), dict(k=17), dict(k=0), dict(stride=0), dict(n=9), dict(n=0))
    for kw in refused:
        assert call(**kw) == UNSUPPORTED and b"served" in lib.emo_last_error_string(), kw
    for kw in (dict(ldy=504), dict(ldy=516), dict(act=3), dict(y=fake + 8), dict(g=fake + 4)):
        assert call(**kw) == BAD_SHAPE, kw
    # the host-only query: the same shape check, a plan on success, nothing written on a refusal
    plan = (C.c_int64 * 6)(*[-1] * 6)
    for kw in refused:
        a = dict(n=16000, Cc=512, k=10, stride=5)
        a.update(kw)
        assert lib.emo_wav_conv0_ln_act_plan(a["n"], a["Cc"], a["k"], a["stride"], plan) == UNSUPPORTED and list(plan) == [-1] * 6
        assert not ops.wav_conv0_ln_act_ok(a["n"], a["Cc"], a["k"], a["stride"])
    assert lib.emo_wav_conv0_ln_act_plan(16000, 512, 10, 5, None) == NULL
    assert lib.emo_wav_conv0_ln_act_plan(16000, 512, 10, 5, plan) == 0
    assert list(plan)[:4] == [3199, 64, 1, 10] and plan[4] >= 1 and plan[5] * 4 * plan[4] >= 3199     # rows, lanes per row, vectors, taps
    assert lib.emo_wav_conv0_ln_act_plan(48000, 1024, 16, 1, plan) == 0 and list(plan)[:4] == [47985, 64, 2, 16]
    assert lib.emo_wav_conv0_ln_act_plan(10, 32, 10, 5, plan) == 0 and list(plan)[:4] == [1, 8, 1, 10]
    assert ops.wav_conv0_ln_act_ok(16000, 512, 10, 5) and ops.wav_conv0_ln_act_ok(3, 40, 3, 2)
