"""The torch-module-like surface every model class takes from emote_hack_amd.module.HipModule (no GPU): one parametrised walk over tiny
instances of each class - what load_state_dict accepts, refuses and accumulates, the state_dict round trip, and what `.to()` parses."""
import pytest
import torch

from emote_hack_amd._lib import EmoHipError
from tests import cases

CLIP_TINY = dict(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4)
POSITION_IDS = torch.arange(8)[None]


def _weights(shapes):
    """f32 tensors that differ from key to key (cheap: the values only have to survive a round trip under the right name)"""
    return {k: torch.full(tuple(s), i + 0.5) for i, (k, s) in enumerate(shapes.items())}


def _unet():
    from emote_hack_amd.spec import param_shapes
    from emote_hack_amd.unet import UNet3DConditionModel
    make = lambda: UNet3DConditionModel(**cases.TINY)
    return make, _weights(param_shapes(make().spec)), {}


def _vae():
    from emote_hack_amd.vae import VAE_DEFAULTS, AutoencoderKL, vae_param_shapes
    from tests.test_gpu_vae import SMALL
    return (lambda: AutoencoderKL(**SMALL)), _weights(vae_param_shapes(dict(VAE_DEFAULTS, **SMALL))), {}


def _clip_text():
    from emote_hack_amd.clip_text import CLIPTextModel, clip_text_param_shapes
    cfg = dict(CLIP_TINY, vocab_size=16, max_position_embeddings=8)
    return (lambda: CLIPTextModel(cfg)), _weights(clip_text_param_shapes(cfg)), {"text_model.embeddings.position_ids": POSITION_IDS}


def _clip_vision(projection):
    from emote_hack_amd.clip_vision import CLIPVisionModel, CLIPVisionModelWithProjection, clip_vision_param_shapes
    cfg = dict(CLIP_TINY, patch_size=4, image_size=8, projection_dim=16)
    tolerated = {"vision_model.embeddings.position_ids": POSITION_IDS[:, :5]}
    if not projection:      # a with-projection checkpoint read as the bare tower
        tolerated["visual_projection.weight"] = torch.zeros(16, 32)
    cls = CLIPVisionModelWithProjection if projection else CLIPVisionModel
    return (lambda: cls(cfg)), _weights(clip_vision_param_shapes(cfg, projection)), tolerated


def _wav2vec2():
    from emote_hack_amd.wav2vec2 import Wav2Vec2Model, wav2vec2_param_shapes
    return (lambda: Wav2Vec2Model(cases.WAV2VEC2_TINY)), _weights(wav2vec2_param_shapes(cases.WAV2VEC2_TINY)), {"masked_spec_embed": torch.zeros(64)}


def _speed_controller():
    from emote_hack_amd.conditioning import SpeedController
    make = lambda: SpeedController(num_buckets=9, embed_dim=16)
    return make, _weights(make().state_dict_shapes()), {}


CASES = {"unet": _unet, "vae": _vae, "clip_text": _clip_text, "clip_vision": lambda: _clip_vision(False),
         "clip_vision_projection": lambda: _clip_vision(True), "wav2vec2": _wav2vec2, "hip_module": _speed_controller}


@pytest.mark.parametrize("name", list(CASES))
def test_module_surface(name):
    make, sd, tolerated = CASES[name]()
    keys = list(sd)
    assert keys == list(make()._shapes)
    with pytest.raises(EmoHipError, match="no weights loaded"):
        make().state_dict()

    # strict loads: a missing key, a wrong shape, an unexpected key
    with pytest.raises(RuntimeError, match="missing"):
        make().load_state_dict({k: sd[k] for k in keys[:-1]})
    with pytest.raises(RuntimeError, match="size mismatch"):
        make().load_state_dict(dict(sd, **{keys[0]: torch.zeros(tuple(sd[keys[0]].shape) + (2,))}))
    extra = dict(sd, **{"no.such.key": torch.zeros(1)})
    if name == "hip_module":        # the conditioning modules' lenient rule: unexpected keys are reported, never refused
        assert make().load_state_dict(extra) == ([], ["no.such.key"])
    else:
        with pytest.raises(RuntimeError, match="unexpected"):
            make().load_state_dict(extra)
    assert make().load_state_dict(extra, strict=False) == ([], ["no.such.key"])
    assert make().load_state_dict(dict(sd, **tolerated)) == ([], [])

    # two complementary strict=False halves accumulate into a complete master, which round-trips bit-exactly
    m = make()
    assert m.load_state_dict({k: sd[k] for k in keys[0::2]}, strict=False) == (keys[1::2], [])
    assert m._absent_keys() == keys[1::2]
    assert m.load_state_dict({k: sd[k] for k in keys[1::2]}, strict=False) == (keys[0::2], [])
    assert m._absent_keys() == [] and m._w is None
    got = m.state_dict()
    assert list(got) != [] and set(got) == set(keys) and all(torch.equal(got[k], sd[k]) and got[k].dtype == torch.float32 for k in keys)

    # .to(): positional and keyword device / dtype in any order; an unsupported dtype is refused there and changes nothing
    cpu = torch.device("cpu")
    assert m.to("cpu") is m and (m.device, m.dtype) == (cpu, torch.float32)
    assert m.to(torch.bfloat16) is m and (m.device, m.dtype) == (cpu, torch.bfloat16)
    assert m.to(device=cpu, dtype=torch.float32) is m and (m.device, m.dtype) == (cpu, torch.float32)
    assert m.to("cpu", torch.float16) is m and (m.device, m.dtype) == (cpu, torch.float16)
    with pytest.raises(EmoHipError, match="float64"):
        m.to(torch.float64)
    assert (m.device, m.dtype) == (cpu, torch.float16) and m._w is None
    assert m.eval() is m and m.requires_grad_(False) is m
    got = m.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in keys)
