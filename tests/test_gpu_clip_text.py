"""GPU parity of the CLIP text encoder (EMOAnimationPipeline._encode_prompt, :202-289): the causal emo_attention against torch,
quick_gelu and the token + position embedding, the HIP CLIPTextModel against the outputs of transformers' own CLIPTextModel on the same
name-keyed weights (tests/golden/clip_text.safetensors, tools/oracle/gen_golden_clip.py), and the pipeline called by prompt string.
f32 mode at rtol 1e-3 / atol 1e-4; bf16 / fp16 against the same f32 goldens at a stated yardstick (below)."""
import json
import os

import pytest
import torch
from safetensors.torch import load_file

from emote_hack_amd.synth import seeded_randn
from tests import cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# the kernel-level tolerances of tests/test_gpu_kernels.py
TOL = {torch.float32: dict(rtol=1e-3, atol=1e-4), torch.bfloat16: dict(rtol=3e-2, atol=3e-2), torch.float16: dict(rtol=5e-3, atol=5e-3)}


@pytest.fixture(scope="module")
def gold():
    return load_file(os.path.join(cases.GOLDEN_DIR, "clip_text.safetensors"))


def _configs():
    with open(os.path.join(cases.GOLDEN_DIR, "clip_text.json")) as f:
        return json.load(f)["configs"]


def _q(t, dtype):
    return t.to(dtype).float()


def _causal_ref(qq, kk, vv, heads, d):
    B, L, _ = qq.shape
    sp = lambda t: t.reshape(B, L, heads, d).permute(0, 2, 1, 3)
    s = torch.matmul(sp(qq), sp(kk).transpose(-1, -2)) * d ** -0.5
    s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float("-inf"))
    return torch.matmul(s.softmax(-1), sp(vv)).permute(0, 2, 1, 3).reshape(B * L, heads * d)


def _causal_run(B, L, heads, d, dtype, seed=60):
    from emote_hack_amd import ops
    C_ = heads * d
    qq, kk, vv = (_q(seeded_randn((B, L, C_), seed + i), dtype) for i in range(3))
    ld = (L + 7) // 8 * 8
    vt = torch.full((B, C_, ld), float("nan"))            # pad columns must never be read into a result
    vt[:, :, :L] = vv.permute(0, 2, 1)
    got = ops.attention(qq.reshape(-1, C_).to(DEV).to(dtype), kk.reshape(-1, C_).to(DEV).to(dtype), vt.to(DEV).to(dtype), L, B=B, Lq=L,
                        heads=heads, d=d, scale=d ** -0.5, causal=True)
    return got.float().cpu(), _causal_ref(qq, kk, vv, heads, d)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [40, 64, 80])
@pytest.mark.parametrize("L", [1, 7, 63, 64, 65, 77, 128, 129, 300, 1000])
def test_causal_attention_vs_torch(L, d, dtype):
    """query row i sees keys j <= i: across the 64-key tile and 128-query block edges; B = 2, 12 heads."""
    got, ref = _causal_run(2, L, 12, d, dtype)
    torch.testing.assert_close(got, ref, **TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [150, 192])
def test_causal_attention_resident_walk(L, dtype):
    """B * heads = 192 (b, head) pairs of two 128-query tiles over <= 3 KV tiles: the launch picks the resident walk (several q tiles
    per block, one ring fill; bf16 / fp16) - every q tile has its own diagonal."""
    got, ref = _causal_run(16, L, 12, 64, dtype, seed=70)
    torch.testing.assert_close(got, ref, **TOL[dtype])


def test_causal_attention_large_scores():
    """Scores spread over many units: the thresholded online softmax must start every row at key 0 (tile 0 first) - a masked
    tile seen first would contribute exp2(0) per key."""
    from emote_hack_amd import ops
    B, L, heads, d = 2, 200, 4, 64
    C_ = heads * d
    qq, kk, vv = (seeded_randn((B, L, C_), 80 + i) * s for i, s in enumerate((4.0, 4.0, 1.0)))
    vt = torch.zeros(B, C_, (L + 7) // 8 * 8)
    vt[:, :, :L] = vv.permute(0, 2, 1)
    got = ops.attention(qq.reshape(-1, C_).to(DEV), kk.reshape(-1, C_).to(DEV), vt.to(DEV), L, B=B, Lq=L, heads=heads, d=d,
                        scale=d ** -0.5, causal=True)
    torch.testing.assert_close(got.cpu(), _causal_ref(qq, kk, vv, heads, d), rtol=1e-3, atol=1e-4)


def test_causal_attention_refusals():
    from emote_hack_amd import ops
    from emote_hack_amd._lib import EmoHipError
    B, L, heads, d = 2, 16, 2, 64
    C_ = heads * d
    x = torch.randn(B * L, C_, device=DEV)
    vt = torch.randn(B, C_, L, device=DEV)
    with pytest.raises(EmoHipError, match="causal"):          # a second KV segment
        ops.attention(x, x, vt, L, B=B, Lq=L, heads=heads, d=d, scale=0.125, causal=True, k1=x, v1t=vt, Lk1=L)
    with pytest.raises(EmoHipError, match="causal"):          # Lq != Lk0
        ops.attention(x[:B * 8], x, vt, L, B=B, Lq=8, heads=heads, d=d, scale=0.125, causal=True)
    # the same calls without the flag run
    ops.attention(x[:B * 8], x, vt, L, B=B, Lq=8, heads=heads, d=d, scale=0.125)


@pytest.mark.parametrize("dtype", DTYPES)
def test_quick_gelu(dtype):
    from emote_hack_amd import ops
    x = _q(seeded_randn((3001,), 90) * 4, dtype)
    got = ops.act(x.to(DEV).to(dtype), "quick_gelu").float().cpu()
    ref = (x * torch.sigmoid(1.702 * x)).to(dtype).float()        # f32 math, rounded once
    torch.testing.assert_close(got, ref, rtol=1e-5 if dtype == torch.float32 else 1e-2, atol=1e-6 if dtype == torch.float32 else 1e-2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_text_embed(dtype):
    from emote_hack_amd import ops
    V, P, D = 300, 20, 96
    tok, pos = _q(seeded_randn((V, D), 91), dtype), _q(seeded_randn((P, D), 92), dtype)
    ids = torch.randint(0, V, (3, 17), generator=torch.Generator().manual_seed(93))
    ids[0, 0], ids[1, 5] = 0, V - 1
    got = ops.text_embed(ids, tok.to(DEV).to(dtype), pos.to(DEV).to(dtype)).float().cpu()
    ref = (torch.nn.functional.embedding(ids, tok) + pos[:17]).to(dtype).float().reshape(-1, D)
    assert torch.equal(got, ref)
    for bad in (V, -1):
        ids2 = ids.clone()
        ids2[2, 3] = bad
        with pytest.raises(IndexError):
            ops.text_embed(ids2, tok.to(DEV).to(dtype), pos.to(DEV).to(dtype))
    with pytest.raises(IndexError):
        ops.text_embed(torch.zeros(1, P + 1, dtype=torch.int64), tok.to(DEV).to(dtype), pos.to(DEV).to(dtype))


_MODELS = {}


def _model(name, dtype, **over):
    from emote_hack_amd.clip_text import CLIPTextModel, clip_text_synth_state_dict
    key = (name, dtype, tuple(sorted(over.items())))
    if key not in _MODELS:
        cfg = dict(_configs()[name], **over)
        m = CLIPTextModel(cfg)
        m.load_state_dict(clip_text_synth_state_dict(_configs()[name]))
        _MODELS[key] = m.to(DEV, dtype)
    return _MODELS[key]


def test_tiny_vs_transformers_f32(gold):
    ids = gold["tiny/input_ids"]
    out = _model("tiny", torch.float32)(ids)
    assert out[0] is out.last_hidden_state and out.last_hidden_state.shape == (2, 16, 64) and out.pooler_output.shape == (2, 64)
    torch.testing.assert_close(out.last_hidden_state.cpu(), gold["tiny/last_hidden_state"], rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(out.pooler_output.cpu(), gold["tiny/pooler_output"], rtol=1e-3, atol=1e-4)       # first EOS (id 500)
    legacy = _model("tiny", torch.float32, eos_token_id=2)(ids.to(DEV))                                         # argmax of the ids
    torch.testing.assert_close(legacy.pooler_output.cpu(), gold["tiny/pooler_output_eos2"], rtol=1e-3, atol=1e-4)
    # an all-ones attention mask and the default position ids are accepted and change nothing
    same = _model("tiny", torch.float32)(ids, attention_mask=torch.ones_like(ids), position_ids=torch.arange(16)[None])
    assert torch.equal(same.last_hidden_state, out.last_hidden_state)


# bf16 / fp16 yardstick: transformers' own CLIPTextModel run in bf16 / fp16 (torch 2.10, CPU) on these weights and ids is off the f32
# golden by (last_hidden_state; the worse of L = 77 and L = 12) bf16 mean 9.6e-3 / max 7.0e-2, fp16 mean 1.2e-3 / max 9.2e-3
# (profiles/clip_text_encode.md); the HIP path may not be worse than 2x the mean / 2.5x the max
LOWP = {torch.bfloat16: (2 * 9.6e-3, 2.5 * 7.0e-2), torch.float16: (2 * 1.2e-3, 2.5 * 9.2e-3)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["sd15", "short"])
def test_sd15_vs_transformers_golden(gold, case, dtype):
    """The SD-1.5 text encoder (12 layers of 12 heads x 64, 77 positions): B = 2 at L = 77 (max_length padding) and L = 12
    (padding="longest"), both pooling rules; last_hidden_state / pooler_output come back in the model's dtype."""
    ids = gold[f"{case}/input_ids"]
    out = _model("sd15", dtype)(ids)
    L = ids.shape[1]
    assert out.last_hidden_state.shape == (2, L, 768) and out.last_hidden_state.dtype == dtype and out.pooler_output.dtype == dtype
    y, p = out.last_hidden_state.float().cpu(), out.pooler_output.float().cpu()
    if dtype == torch.float32:
        torch.testing.assert_close(y, gold[f"{case}/last_hidden_state"], rtol=1e-3, atol=1e-4)
        torch.testing.assert_close(p, gold[f"{case}/pooler_output_eos2"], rtol=1e-3, atol=1e-4)
        if case == "sd15":
            p2 = _model("sd15", dtype, eos_token_id=49407)(ids).pooler_output.cpu()
            torch.testing.assert_close(p2, gold["sd15/pooler_output_eos49407"], rtol=1e-3, atol=1e-4)
    else:
        e = (y - gold[f"{case}/last_hidden_state"]).abs()
        ep = (p - gold[f"{case}/pooler_output_eos2"]).abs()
        tol_mean, tol_max = LOWP[dtype]
        print(f"clip {case} {dtype}: mean err {float(e.mean()):.3e} max {float(e.max()):.3e} pooled max {float(ep.max()):.3e}")
        assert float(e.mean()) < tol_mean and float(e.max()) < tol_max and float(ep.max()) < tol_max


# ---------------------------------------------------------------- end to end: the pipeline called by prompt string
class StubTokenizer:
    """CLIPTokenizer's call interface over a character vocabulary (id = ord % 90 + 3; BOS 1, EOS 2, EOS padding)."""
    model_max_length = 8

    def __call__(self, text, padding="max_length", max_length=None, truncation=False, return_tensors="pt"):
        from types import SimpleNamespace
        seqs = [[1] + [ord(ch) % 90 + 3 for ch in t] + [2] for t in ([text] if isinstance(text, str) else text)]
        if truncation and max_length is not None:
            seqs = [s[:max_length - 1] + [2] if len(s) > max_length else s for s in seqs]
        n = max_length if padding == "max_length" else max(len(s) for s in seqs)
        ids = torch.tensor([s + [2] * (n - len(s)) for s in seqs], dtype=torch.int64)
        return SimpleNamespace(input_ids=ids, attention_mask=torch.ones_like(ids))

    def batch_decode(self, ids):
        return [str(r.tolist()) for r in ids]


def test_pipeline_by_prompt_string():
    """`pipeline(prompt, negative_prompt=...)` with the HIP CLIPTextModel (hidden 32 = the tiny UNet's cross-attention width) and a stub
    tokenizer == the same call with text_embeddings= from _encode_prompt, bit for bit; a second prompt on the reused plan differs from
    the first and equals a fresh pipeline's call."""
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.clip_text import CLIPTextModel, clip_text_synth_state_dict
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    from emote_hack_amd.spec import param_shapes
    from emote_hack_amd.synth import synth_state_dict
    from emote_hack_amd.unet import UNet3DConditionModel

    def build(cfg, prefix="", cls=UNet3DConditionModel, **kw):
        m = cls(**cfg, **kw)
        m.load_state_dict(synth_state_dict(param_shapes(m.spec), prefix=prefix))
        return m.to(DEV, torch.float32)

    ref = build(cases.TINY, cases.REF_PREFIX, cls=AppearanceEncoderModel, _has_out=False)
    unet = build(cases.TINY_MOTION)
    ccfg = dict(vocab_size=100, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4, max_position_embeddings=8,
                eos_token_id=2)
    enc = CLIPTextModel(ccfg)
    enc.load_state_dict(clip_text_synth_state_dict(ccfg))
    enc.to(DEV)

    def pipe():
        return EMOAnimationPipeline(text_encoder=enc, tokenizer=StubTokenizer(), unet=unet, scheduler=DDIMScheduler())

    lat, refl = seeded_randn((1, 4, 8, 16, 16), 5), seeded_randn((1, 4, 16, 16), 3)
    base = dict(video_length=8, height=128, width=128, output_type="latent", appearance_encoder=ref, seed=0, num_inference_steps=3,
                guidance_scale=7.5, context_frames=4, context_stride=1, context_overlap=2, ref_image_latents=refl)
    kw = lambda: dict(base, latents=lat.to(DEV))
    p = pipe()
    out = p("a cat", negative_prompt="blur", **kw()).videos
    text = p._encode_prompt("a cat", DEV, 1, True, "blur")
    assert text.shape == (2, 8, 32) and torch.equal(text[0], p._encode_prompt("blur", DEV, 1, False, None)[0])
    want = pipe()("a cat", text_embeddings=text, **kw()).videos
    assert torch.equal(out, want)
    # another prompt on the kept plan: the new embeddings are bound (not the first call's)
    st = p._plan_cache[1]
    out2 = p("a dog", negative_prompt="blur", **kw()).videos
    assert p._plan_cache[1] is st
    assert not torch.equal(out2, out)
    fresh = pipe()("a dog", negative_prompt="blur", **kw()).videos
    assert torch.equal(out2, fresh)
