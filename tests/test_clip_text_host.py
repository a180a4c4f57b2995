"""Host-side checks of the CLIP text encoder and of the pipeline's prompt encoding (no GPU): the state-dict surface against transformers'
key set (tests/golden/clip_text.json), local checkpoint loading, the refusals, and `_encode_prompt`
(EMOAnimationPipeline.py:202-289) with a stub tokenizer and a stub encoder."""
import json
import logging
import os
from types import SimpleNamespace

import pytest
import torch

from emote_hack_amd.clip_text import SD15_CONFIG, CLIPTextModel, clip_text_param_shapes, clip_text_synth_state_dict
from tests import cases


def _gold_json():
    with open(os.path.join(cases.GOLDEN_DIR, "clip_text.json")) as f:
        return json.load(f)


def test_param_shapes_equal_transformers_key_set():
    g = _gold_json()
    want = {k: tuple(v) for k, v in g["param_shapes"].items()}
    assert {k: tuple(v) for k, v in clip_text_param_shapes().items()} == want
    assert {k: tuple(v) for k, v in clip_text_param_shapes(g["configs"]["sd15"]).items()} == want
    assert g["configs"]["sd15"] == SD15_CONFIG


def test_load_state_dict_tolerates_position_ids_and_checks_keys():
    cfg = _gold_json()["configs"]["tiny"]
    sd = clip_text_synth_state_dict(cfg)
    m = CLIPTextModel(cfg)
    sd["text_model.embeddings.position_ids"] = torch.arange(cfg["max_position_embeddings"])[None]
    missing, unexpected = m.load_state_dict(sd)
    assert missing == [] and unexpected == []
    bad = dict(sd, **{"text_model.encoder.layers.9.mlp.fc1.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="unexpected"):
        CLIPTextModel(cfg).load_state_dict(bad)
    short = {k: v for k, v in sd.items() if "final_layer_norm" not in k}
    with pytest.raises(RuntimeError, match="missing"):
        CLIPTextModel(cfg).load_state_dict(short)
    wrong = dict(sd, **{"text_model.final_layer_norm.weight": torch.ones(3)})
    with pytest.raises(RuntimeError, match="size mismatch"):
        CLIPTextModel(cfg).load_state_dict(wrong)


def test_config_defaults_and_activation():
    m = CLIPTextModel()
    assert (m.config.vocab_size, m.config.hidden_size, m.config.num_hidden_layers, m.config.num_attention_heads,
            m.config.intermediate_size, m.config.max_position_embeddings, m.config.hidden_act, m.config.layer_norm_eps) == \
        (49408, 768, 12, 12, 3072, 77, "quick_gelu", 1e-5)
    assert CLIPTextModel(SimpleNamespace(hidden_act="gelu", hidden_size=64, num_attention_heads=4)).config.hidden_act == "gelu"
    with pytest.raises(NotImplementedError):
        CLIPTextModel(hidden_act="relu")


def test_from_pretrained_reads_a_local_folder(tmp_path):
    from safetensors.torch import save_file
    cfg = _gold_json()["configs"]["tiny"]
    sd = clip_text_synth_state_dict(cfg)
    d = tmp_path / "text_encoder"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(dict(cfg, architectures=["CLIPTextModel"], model_type="clip_text_model",
                                                   projection_dim=768, torch_dtype="float32")))
    save_file(dict(sd, **{"text_model.embeddings.position_ids": torch.arange(cfg["max_position_embeddings"])[None]}),
              str(d / "model.safetensors"))
    m = CLIPTextModel.from_pretrained(str(tmp_path), subfolder="text_encoder")
    assert m.config.hidden_size == 64 and m.config.eos_token_id == cfg["eos_token_id"]
    assert all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    # pytorch_model.bin when there is no safetensors file
    os.remove(d / "model.safetensors")
    torch.save(sd, str(d / "pytorch_model.bin"))
    m2 = CLIPTextModel.from_pretrained(str(tmp_path))
    assert all(torch.equal(m2.state_dict()[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError, match="does not exist"):
        CLIPTextModel.from_pretrained(str(tmp_path / "nowhere"))


def test_forward_refusals_before_any_launch():
    cfg = _gold_json()["configs"]["tiny"]
    m = CLIPTextModel(cfg)
    m.load_state_dict(clip_text_synth_state_dict(cfg))
    m._w = {}      # past the "weights packed" gate: these checks run on the host before the first launch
    ids = torch.ones(2, 8, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="attention mask"):
        m(ids, attention_mask=torch.tensor([[1] * 8, [1] * 6 + [0] * 2]))
    with pytest.raises(NotImplementedError, match="position_ids"):
        m(ids, position_ids=torch.arange(8).flip(0)[None])
    with pytest.raises(NotImplementedError, match="clip-skip"):
        m(ids, output_hidden_states=True)
    with pytest.raises(ValueError, match="sequence length"):
        m(torch.ones(1, cfg["max_position_embeddings"] + 1, dtype=torch.int64))


# ---------------------------------------------------------------- _encode_prompt with stubs
class StubTokenizer:
    """CLIPTokenizer's call interface: one id per character (ord % 90 + 3), BOS 1, EOS 2, EOS padding."""
    model_max_length = 8

    def __init__(self):
        self.calls = []

    def _ids(self, text):
        return [1] + [ord(ch) % 90 + 3 for ch in text] + [2]

    def __call__(self, text, padding="max_length", max_length=None, truncation=False, return_tensors="pt"):
        texts = [text] if isinstance(text, str) else list(text)
        self.calls.append((tuple(texts), padding, max_length, truncation))
        seqs = [self._ids(t) for t in texts]
        if truncation and max_length is not None:
            seqs = [s[:max_length - 1] + [2] if len(s) > max_length else s for s in seqs]
        n = max_length if padding == "max_length" else max(len(s) for s in seqs)
        ids = torch.tensor([s + [2] * (n - len(s)) for s in seqs], dtype=torch.int64)
        return SimpleNamespace(input_ids=ids, attention_mask=torch.ones_like(ids))

    def batch_decode(self, ids):
        return ["".join(chr(int(i)) for i in row) for row in ids]


class StubEncoder:
    """embedding row (b, l) = id * 10 + l, in D = 3 channels; records its calls."""
    config = SimpleNamespace()

    def __init__(self):
        self.calls = []

    def __call__(self, input_ids, attention_mask=None):
        self.calls.append((input_ids.clone(), attention_mask))
        L = input_ids.shape[1]
        e = (input_ids.float() * 10 + torch.arange(L).float())[..., None].expand(-1, -1, 3).contiguous()
        return (e,)


def _pipe():
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    p = EMOAnimationPipeline.__new__(EMOAnimationPipeline)        # _encode_prompt needs the tokenizer and the encoder only
    p.tokenizer, p.text_encoder = StubTokenizer(), StubEncoder()
    return p


def _emb(p, text, L=8):
    ids = p.tokenizer(text, padding="max_length", max_length=L, truncation=True).input_ids
    return p.text_encoder.__class__()(ids)[0]


def test_encode_prompt_cfg_order_and_default_negative():
    p = _pipe()
    out = p._encode_prompt("cat", "cpu", 1, True, None)
    assert out.shape == (2, 8, 3)
    assert torch.equal(out[0], _emb(p, "")[0]) and torch.equal(out[1], _emb(p, "cat")[0])        # [uncond, cond]
    # the tokenizer was called with the reference's arguments
    assert p.tokenizer.calls[0] == (("cat",), "max_length", 8, True)
    assert p.tokenizer.calls[1] == (("cat",), "longest", None, False)
    assert p.tokenizer.calls[2] == (("",), "max_length", 8, True)
    neg = p._encode_prompt("cat", "cpu", 1, True, "dog")
    assert torch.equal(neg[0], _emb(p, "dog")[0]) and torch.equal(neg[1], out[1])
    lst = p._encode_prompt(["cat"], "cpu", 1, True, ["dog"])
    assert torch.equal(lst, neg)


def test_encode_prompt_without_guidance_and_per_prompt_copies():
    p = _pipe()
    one = p._encode_prompt("cat", "cpu", 1, False, "ignored")
    assert one.shape == (1, 8, 3) and torch.equal(one[0], _emb(p, "cat")[0])
    two = p._encode_prompt(["cat", "ox"], "cpu", 2, True, None)
    assert two.shape == (8, 8, 3)
    want = [_emb(p, t)[0] for t in ("", "", "", "", "cat", "cat", "ox", "ox")]
    assert all(torch.equal(two[i], w) for i, w in enumerate(want))


def test_encode_prompt_negative_prompt_errors():
    p = _pipe()
    with pytest.raises(TypeError, match="same type"):
        p._encode_prompt("cat", "cpu", 1, True, ["dog"])
    with pytest.raises(ValueError, match="batch size"):
        p._encode_prompt(["cat"], "cpu", 1, True, ["dog", "eel"])


def test_encode_prompt_warns_on_truncation(caplog):
    p = _pipe()
    with caplog.at_level(logging.WARNING, logger="emote_hack_amd.pipeline"):
        out = p._encode_prompt("a long prompt", "cpu", 1, True, None)
    assert out.shape == (2, 8, 3)
    assert any("truncated" in r.getMessage() for r in caplog.records)


def test_call_uses_encode_prompt_with_a_tokenizer(monkeypatch):
    """__call__ without text_embeddings=: the tokenizer path calls _encode_prompt(prompt, device, n, guidance_scale > 1, negative_prompt);
    without a tokenizer the old `text_encoder(prompt, negative_prompt)` call stays."""
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
    with pytest.raises(Stop):
        p("cat", 2, negative_prompt="dog", guidance_scale=7.5, **kw)
    assert torch.equal(seen["text"], p._encode_prompt("cat", "cpu", 1, True, "dog"))
    with pytest.raises(Stop):
        p("cat", 2, guidance_scale=1.0, **kw)
    assert seen["text"].shape == (1, 8, 3)
    p.tokenizer = None
    p.text_encoder = lambda prompt, neg: ("legacy", prompt, neg)
    with pytest.raises(Stop):
        p("cat", 2, negative_prompt="dog", **kw)
    assert seen["text"] == ("legacy", "cat", "dog")
