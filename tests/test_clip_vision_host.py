"""Host-side checks of the CLIP vision encoder, its image processor and the pipeline's image conditioning (no GPU): the state-dict
surface against transformers' key set (tests/golden/clip_vision.json), local checkpoint loading, the refusals, the processor's size /
crop arithmetic against transformers' own rule, the tap tables against torch's antialiased bicubic, and `_encode_image` with a stub
encoder."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from emote_hack_amd._lib import EmoHipError
from emote_hack_amd.clip_vision import (OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, VITL14_CONFIG, CLIPImageProcessor, CLIPVisionModel,
                                        CLIPVisionModelWithProjection, center_crop_offsets, clip_vision_param_shapes,
                                        clip_vision_synth_state_dict, resize_crop_taps, resize_output_size)
from tests import cases
from tests.frontend_sweep_cases import IP_CASES

GEOMETRIES = [(512, 512), (480, 640), (768, 512), (300, 200), (224, 224), (225, 301)]      # (H, W); the last has an odd crop difference


def _gold_json():
    with open(os.path.join(cases.GOLDEN_DIR, "clip_vision.json")) as f:
        return json.load(f)


def test_param_shapes_equal_transformers_key_set():
    g = _gold_json()
    want = {k: tuple(v) for k, v in g["param_shapes"].items()}
    assert {k: tuple(v) for k, v in clip_vision_param_shapes().items()} == want
    assert {k: tuple(v) for k, v in clip_vision_param_shapes(g["configs"]["vitl14"]).items()} == want
    assert g["configs"]["vitl14"] == VITL14_CONFIG
    assert "vision_model.pre_layrnorm.weight" in want and "visual_projection.weight" in want            # the upstream spelling
    bare = clip_vision_param_shapes(projection=False)
    assert set(want) - set(bare) == {"visual_projection.weight"}
    assert want["vision_model.embeddings.position_embedding.weight"] == (257, 1024) and want["visual_projection.weight"] == (768, 1024)


def test_config_defaults_and_refused_configs():
    m = CLIPVisionModelWithProjection()
    c = m.config
    assert (c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads, c.image_size, c.patch_size, c.projection_dim,
            c.hidden_act, c.layer_norm_eps) == (1024, 4096, 24, 16, 224, 14, 768, "quick_gelu", 1e-5)
    assert CLIPVisionModel(SimpleNamespace(hidden_act="gelu", hidden_size=64, num_attention_heads=4)).config.hidden_act == "gelu"
    with pytest.raises(NotImplementedError):
        CLIPVisionModel(hidden_act="relu")
    with pytest.raises(ValueError):
        CLIPVisionModel(image_size=225)


def test_load_state_dict_tolerates_position_ids_and_checks_keys():
    cfg = _gold_json()["configs"]["tiny"]
    sd = clip_vision_synth_state_dict(cfg)
    m = CLIPVisionModelWithProjection(cfg)
    sd["vision_model.embeddings.position_ids"] = torch.arange(10)[None]
    missing, unexpected = m.load_state_dict(sd)
    assert missing == [] and unexpected == []
    assert set(m.state_dict()) == set(clip_vision_param_shapes(cfg))
    bad = dict(sd, **{"vision_model.encoder.layers.9.mlp.fc1.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="unexpected"):
        CLIPVisionModelWithProjection(cfg).load_state_dict(bad)
    short = {k: v for k, v in sd.items() if "pre_layrnorm" not in k}
    with pytest.raises(RuntimeError, match="missing"):
        CLIPVisionModelWithProjection(cfg).load_state_dict(short)
    with pytest.raises(RuntimeError, match="missing"):            # the corrected spelling is NOT the checkpoint's
        CLIPVisionModelWithProjection(cfg).load_state_dict({k.replace("pre_layrnorm", "pre_layernorm"): v for k, v in sd.items()}, strict=True)
    wrong = dict(sd, **{"visual_projection.weight": torch.ones(3, 64)})
    with pytest.raises(RuntimeError, match="size mismatch"):
        CLIPVisionModelWithProjection(cfg).load_state_dict(wrong)
    # the bare tower reads a with-projection checkpoint (the projection is dropped), the other direction misses a key
    assert CLIPVisionModel(cfg).load_state_dict(sd) == ([], [])
    with pytest.raises(RuntimeError, match="missing"):
        CLIPVisionModelWithProjection(cfg).load_state_dict(clip_vision_synth_state_dict(cfg, projection=False))


def test_from_pretrained_reads_a_local_folder(tmp_path):
    from safetensors.torch import save_file
    cfg = _gold_json()["configs"]["tiny"]
    sd = clip_vision_synth_state_dict(cfg)
    d = tmp_path / "image_encoder"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(dict(cfg, architectures=["CLIPVisionModelWithProjection"], model_type="clip_vision_model",
                                                   torch_dtype="float32")))
    save_file(dict(sd, **{"vision_model.embeddings.position_ids": torch.arange(10)[None]}), str(d / "model.safetensors"))
    m = CLIPVisionModelWithProjection.from_pretrained(str(tmp_path))                       # default subfolder: image_encoder
    assert m.config.hidden_size == 64 and m.config.image_size == 42 and m.config.projection_dim == 32
    assert all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    os.remove(d / "model.safetensors")
    torch.save(sd, str(d / "pytorch_model.bin"))
    m2 = CLIPVisionModelWithProjection.from_pretrained(str(tmp_path), subfolder="image_encoder", torch_dtype=torch.bfloat16)
    assert m2.dtype == torch.bfloat16 and all(torch.equal(m2.state_dict()[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError, match="does not exist"):
        CLIPVisionModelWithProjection.from_pretrained(str(tmp_path / "nowhere"))
    os.remove(d / "pytorch_model.bin")
    with pytest.raises(RuntimeError, match="neither"):
        CLIPVisionModelWithProjection.from_pretrained(str(tmp_path))


def test_forward_refusals_before_any_launch():
    cfg = _gold_json()["configs"]["tiny"]
    m = CLIPVisionModelWithProjection(cfg)
    m.load_state_dict(clip_vision_synth_state_dict(cfg))
    with pytest.raises(EmoHipError, match="no CPU execution path"):          # weights loaded, but not on a HIP device
        m(torch.zeros(1, 3, 42, 42))
    m._w = {}      # past the "weights packed" gate: these checks run on the host before the first launch
    x = torch.zeros(2, 3, 42, 42)
    with pytest.raises(NotImplementedError, match="interpolate_pos_encoding"):
        m(x, interpolate_pos_encoding=True)
    with pytest.raises(NotImplementedError, match="output_attentions"):
        m(x, output_attentions=True)
    with pytest.raises(ValueError, match="image_size"):
        m(torch.zeros(2, 3, 56, 56))
    with pytest.raises(ValueError, match="pixel_values"):
        m(torch.zeros(2, 42, 42))


# ---------------------------------------------------------------- the processor's arithmetic
@pytest.mark.parametrize("H,W", GEOMETRIES)
def test_size_and_crop_rule_equals_transformers(H, W):
    from transformers.image_transforms import center_crop, get_resize_output_image_size
    img = np.zeros((3, H, W), dtype=np.uint8)
    want = get_resize_output_image_size(img, size=224, default_to_square=False, input_data_format="channels_first")
    assert resize_output_size(H, W, 224) == tuple(want)
    rh, rw = want
    idx = np.arange(rh * rw, dtype=np.int64).reshape(1, rh, rw)            # every pixel names its own position
    win = center_crop(idx, (224, 224), input_data_format="channels_first")
    top, left = center_crop_offsets(rh, rw, 224)
    assert win.shape == (1, 224, 224) and int(win[0, 0, 0]) == top * rw + left
    g = _gold_json()["processor_definition_vs_pil"].get(f"{H}x{W}")
    if g is not None:
        assert g["resized"] == [rh, rw] and g["crop_top_left"] == [top, left]


# (H, W, S): the geometries above at crop 224, then the table tests/test_gpu_frontend_sweeps.py runs on the device (the first ones keep
# their two-number ids)
_TAP_224 = [(H, W, 224) for H, W in GEOMETRIES + [(100, 160), (1080, 1920)]]
_TAP_CASES = _TAP_224 + [c for c in IP_CASES if c not in _TAP_224]


@pytest.mark.parametrize("H,W,S", _TAP_CASES, ids=[f"{H}-{W}" if i < len(_TAP_224) else f"{H}-{W}-{S}" for i, (H, W, S) in enumerate(_TAP_CASES)])
def test_tap_tables_reproduce_torch_antialiased_bicubic(H, W, S):
    """What emo_image_preprocess computes from the host tables (both passes in f32, numpy here) == the definition: F.interpolate(bicubic,
    antialias=True) to the shortest-edge size, centre crop, clamp, rescale, normalise - enlarging (100x160) and strong shrinking too,
    frames smaller than the filter support, extreme aspect ratios, crops of 32 .. 336."""
    t = resize_crop_taps(H, W, S, S)
    assert t["ytap"].shape == t["xtap"].shape == (S, 2) and t["ytap"].dtype == np.int32 and t["yw"].dtype == np.float32
    for tap, wt, n in ((t["ytap"], t["yw"], H), (t["xtap"], t["xw"], W)):       # inside the frame, weights sum to one
        assert tap[:, 0].min() >= 0 and (tap[:, 0] + tap[:, 1]).max() <= n and tap[:, 1].min() >= 1 and tap[:, 1].max() <= wt.shape[1]
        np.testing.assert_allclose(wt.sum(1), 1.0, atol=1e-5)
        assert all((wt[i, tap[i, 1]:] == 0).all() for i in range(S))
    assert 1 <= t["span_max"] <= W
    img = torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(H * 7 + W), dtype=torch.uint8)
    x = img.numpy().astype(np.float32)
    col = np.stack([(t["yw"][oy, :t["ytap"][oy, 1], None, None] * x[t["ytap"][oy, 0]:t["ytap"][oy, 0] + t["ytap"][oy, 1]]).sum(0) for oy in range(S)])
    out = np.stack([(t["xw"][ox, None, :t["xtap"][ox, 1], None] * col[:, t["xtap"][ox, 0]:t["xtap"][ox, 0] + t["xtap"][ox, 1]]).sum(1)
                    for ox in range(S)], 1)                                 # (S, S, 3)
    got = (np.clip(out, 0, 255) * np.float32(1 / 255) - np.array(OPENAI_CLIP_MEAN, np.float32)) / np.array(OPENAI_CLIP_STD, np.float32)
    rh, rw = t["size"]
    ref = torch.nn.functional.interpolate(img.permute(2, 0, 1)[None].float(), size=(rh, rw), mode="bicubic", antialias=True, align_corners=False)
    ref = ref[0, :, t["top"]:t["top"] + S, t["left"]:t["left"] + S].clamp(0, 255) * (1 / 255)
    ref = (ref - torch.tensor(OPENAI_CLIP_MEAN)[:, None, None]) / torch.tensor(OPENAI_CLIP_STD)[:, None, None]
    torch.testing.assert_close(torch.from_numpy(got).permute(2, 0, 1), ref, rtol=1e-4, atol=2e-5)


def test_processor_surface_and_refusals():
    p = CLIPImageProcessor()
    assert p.size == {"shortest_edge": 224} and p.crop_size == {"height": 224, "width": 224} and p.do_convert_rgb and p.resample == 3
    assert tuple(p.image_mean) == OPENAI_CLIP_MEAN and tuple(p.image_std) == OPENAI_CLIP_STD
    assert CLIPImageProcessor(size=42, crop_size={"height": 42, "width": 42}).size == {"shortest_edge": 42}
    with pytest.raises(NotImplementedError):
        CLIPImageProcessor(size={"height": 224, "width": 224})
    with pytest.raises(NotImplementedError):
        CLIPImageProcessor(resample=2)
    with pytest.raises(ValueError, match="smaller"):
        resize_crop_taps(100, 100, 64, 96)
    # grouping of the accepted inputs (no launch): one array, a list, a batch, a PIL image
    from PIL import Image
    a, b = np.zeros((30, 40, 3), np.uint8), np.zeros((50, 40, 3), np.uint8)
    shapes = lambda x: [tuple(t.shape) for t in p._frames(x)]
    assert shapes(a) == [(1, 30, 40, 3)] and shapes(torch.from_numpy(a)) == [(1, 30, 40, 3)]
    assert shapes([a, a, b]) == [(2, 30, 40, 3), (1, 50, 40, 3)]
    assert shapes(np.zeros((4, 30, 40, 3), np.uint8)) == [(4, 30, 40, 3)]
    assert shapes(Image.fromarray(a).convert("L")) == [(1, 30, 40, 3)]         # do_convert_rgb
    with pytest.raises(ValueError, match="uint8"):
        p._frames(np.zeros((30, 40, 3), np.float32))
    if not torch.cuda.is_available():
        with pytest.raises(EmoHipError):
            CLIPImageProcessor(device="cpu")(a)


# ---------------------------------------------------------------- _encode_image with stubs
class StubProcessor:
    def __init__(self):
        self.calls = 0

    def __call__(self, images, return_tensors="pt"):
        self.calls += 1
        im = torch.as_tensor(images).float()
        return SimpleNamespace(pixel_values=im.mean().reshape(1, 1, 1, 1).expand(1, 3, 4, 4).contiguous())


class StubImageEncoder:
    """image_embeds = (mean pixel value + 1) * [1, 2, 3, 4, 5]"""
    config = SimpleNamespace(image_size=4, projection_dim=5)

    def __init__(self):
        self.seen = []

    def __call__(self, pixel_values):
        self.seen.append(pixel_values)
        e = (pixel_values.float().mean(dim=(1, 2, 3))[:, None] + 1) * torch.arange(1, 6).float()[None]
        return SimpleNamespace(image_embeds=e)


def _pipe():
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    p = EMOAnimationPipeline.__new__(EMOAnimationPipeline)
    p.tokenizer, p.text_encoder = None, None
    p.image_encoder, p.image_processor = StubImageEncoder(), StubProcessor()
    return p


def test_encode_image_cfg_order_zero_uncond_and_pixel_values_passthrough():
    p = _pipe()
    img = np.full((6, 8, 3), 10, np.uint8)
    two = p._encode_image(img, "cpu", 1, True)
    assert two.shape == (2, 1, 5) and p.image_processor.calls == 1
    assert torch.equal(two[0], torch.zeros(1, 5)) and torch.equal(two[1, 0], 11 * torch.arange(1, 6).float())       # [uncond, cond]
    one = p._encode_image(img, "cpu", 1, False)
    assert one.shape == (1, 1, 5) and torch.equal(one[0], two[1])
    pv = torch.full((1, 3, 4, 4), 2.0)                                      # already pixel_values: the processor is not called
    direct = p._encode_image(pv, "cpu", 1, True)
    assert p.image_processor.calls == 2 and torch.equal(direct[1, 0], 3 * torch.arange(1, 6).float())
    assert p._encode_image(pv, "cpu", 2, True).shape == (4, 1, 5)


def test_ctor_takes_image_encoder_and_builds_the_default_processor():
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    unet = SimpleNamespace(device=torch.device("cpu"))
    p = EMOAnimationPipeline(None, None, None, unet, None, DDIMScheduler())                 # the positional order is unchanged
    assert p.image_encoder is None and p.image_processor is None
    enc = SimpleNamespace(config=SimpleNamespace(image_size=42), device=torch.device("cpu"))
    p = EMOAnimationPipeline(unet=unet, scheduler=DDIMScheduler(), image_encoder=enc)
    assert isinstance(p.image_processor, CLIPImageProcessor) and p.image_processor.size == {"shortest_edge": 42}
    assert p.image_processor.crop_size == {"height": 42, "width": 42}
    mine = StubProcessor()
    assert EMOAnimationPipeline(unet=unet, scheduler=DDIMScheduler(), image_encoder=enc, image_processor=mine).image_processor is mine


def test_call_with_clip_image(monkeypatch):
    """__call__(..., clip_image=) takes the context from _encode_image; with a prompt, with text_embeddings= or without an image encoder
    it is a ValueError; without clip_image the prompt path is untouched."""
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    seen = {}

    class Stop(Exception):
        pass

    def fake_denoise(self, lat, ref, text, **kw):
        seen["text"] = text
        raise Stop

    monkeypatch.setattr(EMOAnimationPipeline, "denoise", fake_denoise)
    p = _pipe()
    p.unet = SimpleNamespace(config=SimpleNamespace(sample_size=2), device=torch.device("cpu"), in_channels=4)
    p.controlnet, p.vae, p.vae_scale_factor = None, None, 8
    p.scheduler = SimpleNamespace(init_noise_sigma=1.0)
    kw = dict(appearance_encoder=object(), ref_image_latents=torch.zeros(1, 4, 2, 2), latents=torch.zeros(1, 4, 2, 2, 2))
    img = np.full((6, 8, 3), 10, np.uint8)
    with pytest.raises(Stop):
        p("", 2, guidance_scale=7.5, clip_image=img, **kw)
    assert torch.equal(seen["text"], p._encode_image(img, "cpu", 1, True))
    with pytest.raises(Stop):
        p("", 2, guidance_scale=1.0, clip_image=img, **kw)
    assert seen["text"].shape == (1, 1, 5)
    with pytest.raises(ValueError, match="prompt"):
        p("a cat", 2, clip_image=img, **kw)
    with pytest.raises(ValueError, match="text_embeddings"):
        p("", 2, clip_image=img, text_embeddings=torch.zeros(2, 1, 5), **kw)
    p.image_encoder = None
    with pytest.raises(ValueError, match="image_encoder"):
        p("", 2, clip_image=img, **kw)
    with pytest.raises(ValueError, match="text_embeddings"):              # the old message of a pipeline without any encoder
        p("", 2, **kw)
