"""CPU tests of the two UNet3DConditionModel ctor switches no shipped config turns on - unet_use_temporal_attention=True (attn_temp,
attention.py:235-246,309-318) and resnet_time_scale_shift="scale_shift" (resnet.py:149-156,191-195): the config surface, the state-dict
keys against the listing captured from the reference models (tests/golden/unet_switches2.json, tools/oracle/gen_golden_switches2.py), the
refusals that stay, and the coefficient algebra of the modulated GroupNorm (emo_hip.h emo_groupnorm_coeffs_mod)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from emote_hack_amd.config import normalize_unet_config
from emote_hack_amd.spec import build_spec, param_shapes
from emote_hack_amd.synth import seeded_randn
from tests import cases

TEMP = dict(unet_use_temporal_attention=True)
SS = dict(resnet_time_scale_shift="scale_shift")


@pytest.fixture(scope="module")
def listing():
    return json.load(open(os.path.join(cases.GOLDEN_DIR, "unet_switches2.json")))


@pytest.mark.parametrize("name,base", [("both_keys", cases.TINY_MOTION), ("both_linear_keys", cases.TINY_LINEAR)])
def test_state_dict_keys_match_the_reference_listing(listing, name, base):
    """names, shapes AND registration order of the reference model with both switches on"""
    mine = param_shapes(build_spec(dict(base, **TEMP, **SS)))
    want = listing[name]
    assert {k: list(v) for k, v in mine.items()} == want
    assert sorted(mine) == sorted(want)
    # the new keys: 16 transformer blocks x (to_q, to_k, to_v, to_out.0.weight, to_out.0.bias, norm_temp.weight, norm_temp.bias)
    assert sum(1 for k in mine if ".attn_temp." in k or ".norm_temp." in k) == 112
    c = base["block_out_channels"][0]
    assert mine["down_blocks.0.resnets.0.time_emb_proj.weight"] == (2 * c, 4 * c)
    assert mine["down_blocks.0.resnets.0.time_emb_proj.bias"] == (2 * c,)
    tb = "down_blocks.0.attentions.0.transformer_blocks.0"
    assert mine[tb + ".attn_temp.to_q.weight"] == (c, c) and mine[tb + ".attn_temp.to_out.0.bias"] == (c,) and mine[tb + ".norm_temp.weight"] == (c,)


def test_one_switch_changes_only_its_own_keys():
    plain = param_shapes(build_spec(cases.TINY_MOTION))
    temp = param_shapes(build_spec(dict(cases.TINY_MOTION, **TEMP)))
    ss = param_shapes(build_spec(dict(cases.TINY_MOTION, **SS)))
    assert {k: v for k, v in temp.items() if ".attn_temp." not in k and ".norm_temp." not in k} == dict(plain)
    assert list(ss) == list(plain)
    changed = [k for k in ss if ss[k] != plain[k]]
    n_resnets = sum(1 for k in plain if k.endswith(".time_emb_proj.weight"))
    assert len(changed) == 2 * n_resnets and all(".time_emb_proj." in k for k in changed)
    assert all(ss[k][0] == 2 * plain[k][0] and ss[k][1:] == plain[k][1:] for k in changed)


def test_switches_off_is_the_model_of_before():
    """both switches off (None / False / "default", as every shipped config has them): the key listing of the reference's unswitched model"""
    ints = json.load(open(os.path.join(cases.GOLDEN_DIR, "ints.json")))
    for extra in ({}, dict(unet_use_temporal_attention=False, resnet_time_scale_shift="default"), dict(unet_use_temporal_attention=None)):
        mine = param_shapes(build_spec(dict(cases.TINY_MOTION, **extra)))
        assert {k: list(v) for k, v in mine.items()} == ints["tiny_motion_keys"]
        assert not any("attn_temp" in k or "norm_temp" in k for k in mine)


def test_config_accepts_the_switches_and_rejects_unknown_values():
    cfg = normalize_unet_config(dict(cases.TINY_MOTION, **TEMP, **SS))
    assert cfg["unet_use_temporal_attention"] is True and cfg["resnet_time_scale_shift"] == "scale_shift"
    assert cfg.resnet_time_scale_shift == "scale_shift"
    with pytest.raises(ValueError, match="time_embedding_norm"):      # resnet.py:153-154
        normalize_unet_config(dict(cases.TINY_MOTION, resnet_time_scale_shift="ada_group"))
    with pytest.raises(ValueError):
        build_spec(dict(cases.TINY_MOTION, resnet_time_scale_shift="bogus"))
    # the refusals next to them stay
    with pytest.raises(NotImplementedError):
        normalize_unet_config(dict(cases.TINY_MOTION, dual_cross_attention=True))
    with pytest.raises(NotImplementedError):
        normalize_unet_config(dict(cases.TINY_MOTION, motion_module_kwargs=dict(cases.MOTION_KW_TINY, attention_block_types=["Temporal_Cross"])))


def test_model_ctor_builds_with_the_switches():
    from emote_hack_amd.unet import UNet3DConditionModel
    m = UNet3DConditionModel(**dict(cases.TINY_MOTION, **TEMP, **SS))
    assert all(a.temporal for b in m.spec.down + [m.spec.mid] + m.spec.up for a in b.attentions if a is not None)
    assert all(r.scale_shift and r.temb_cols == 2 * r.cout for b in m.spec.down + [m.spec.mid] + m.spec.up for r in b.resnets)
    m0 = UNet3DConditionModel(**cases.TINY_MOTION)
    assert not any(a.temporal for b in m0.spec.down + [m0.spec.mid] + m0.spec.up for a in b.attentions if a is not None)
    assert not any(r.scale_shift for b in m0.spec.down + [m0.spec.mid] + m0.spec.up for r in b.resnets)


def test_appearance_encoder_refuses_temporal_attention():
    """the reference's ReferenceNet is a 2-D diffusers clone with no attn_temp branch: refuse instead of silently building one"""
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    with pytest.raises(NotImplementedError, match="AppearanceEncoderModel"):
        AppearanceEncoderModel(**dict(cases.TINY, **TEMP))
    AppearanceEncoderModel(**cases.TINY)


def test_controlnet_refuses_scale_shift():
    """ControlNet block arithmetic is third-party: scale_shift stays out of scope, in the ctor and through from_unet"""
    from emote_hack_amd.controlnet import ControlNetModel
    from emote_hack_amd.unet import UNet3DConditionModel
    kw = {k: v for k, v in cases.TINY.items() if not k.startswith("unet_use")}
    with pytest.raises(NotImplementedError, match="ControlNetModel"):
        ControlNetModel(**dict(kw, **SS))
    with pytest.raises(NotImplementedError, match="ControlNetModel"):
        ControlNetModel.from_unet(UNet3DConditionModel(**dict(cases.TINY, **SS)), load_weights_from_unet=False)
    ControlNetModel(**kw)
    ControlNetModel.from_unet(UNet3DConditionModel(**cases.TINY), load_weights_from_unet=False)


@pytest.mark.parametrize("silu", [False, True])
def test_modulated_groupnorm_coefficient_algebra(silu):
    """What emo_groupnorm_coeffs_mod tabulates and emo_groupnorm_apply_mod / emo_groupnorm_mod apply (emo_hip.h): per (instance, channel)
    scale' = rstd gamma (1 + s), shift' = (beta - mean rstd gamma)(1 + s) + t, so that act(x scale' + shift') == act(GN(x) (1 + s) + t) -
    restated in torch f64 against group_norm -> modulate as resnet.py:191-197 writes it (the GPU test holds the kernels to the same)."""
    N, S, C, G, eps = 3, 40, 32, 8, 1e-5
    x = (seeded_randn((N, S, C), 7) * 1.7 + 0.4).double()
    gamma, beta = (1 + 0.1 * seeded_randn((C,), 8)).double(), (0.1 * seeded_randn((C,), 9)).double()
    mod = torch.cat([0.5 * seeded_randn((N, C), 10), seeded_randn((N, C), 11)], 1).double()     # (scale | shift)
    s, t = torch.chunk(mod, 2, dim=1)
    ref = F.group_norm(x.permute(0, 2, 1), G, gamma, beta, eps) * (1 + s[:, :, None]) + t[:, :, None]
    ref = (F.silu(ref) if silu else ref).permute(0, 2, 1)
    xg = x.reshape(N, S, G, C // G)
    mean_c = xg.mean((1, 3)).repeat_interleave(C // G, 1)                                       # (N, C)
    rstd_c = (xg.var((1, 3), unbiased=False) + eps).rsqrt().repeat_interleave(C // G, 1)
    a = rstd_c * gamma[None]
    b = beta[None] - mean_c * a
    a2, b2 = a * (1 + s), b * (1 + s) + t
    got = x * a2[:, None, :] + b2[:, None, :]
    torch.testing.assert_close(F.silu(got) if silu else got, ref, rtol=1e-9, atol=1e-9)
