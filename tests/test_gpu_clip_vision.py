"""GPU parity of the CLIP vision encoder (the `image_encoder` of EMOAnimationPipeline.py:867,909-917): emo_image_preprocess against its
CPU f32 definition and against transformers' own PIL-backed CLIPImageProcessor, emo_patch_rows, emo_vision_embed, the non-causal
emo_attention at the encoder's shapes, the HIP CLIPVisionModelWithProjection against the outputs of transformers' own class on the same
name-keyed weights (tests/golden/clip_vision.safetensors, tools/oracle/gen_golden_clip_vision.py), the pipeline conditioned on an image,
and a VideoNet fed the one-token context.  f32 mode at rtol 1e-3 / atol 1e-4; bf16 / fp16 against the same f32 goldens at the yardstick
of tests/test_gpu_clip_text.py: mean error <= 2x, max error <= 2.5x transformers' own low-precision error (recorded in the .json)."""
import json
import os

import pytest
import torch
from safetensors.torch import load_file

from emote_hack_amd.synth import seeded_randn, synth_state_dict
from tests import cases
from tests.test_gpu_clip_text import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
PROC_SIZES = [(512, 512), (480, 640), (768, 512), (300, 200), (224, 224)]      # (H, W), as the generator lists them
ATOL, RTOL = 1e-4, 1e-3


@pytest.fixture(scope="module")
def gold():
    return load_file(os.path.join(cases.GOLDEN_DIR, "clip_vision.safetensors"))


def _meta():
    with open(os.path.join(cases.GOLDEN_DIR, "clip_vision.json")) as f:
        return json.load(f)


def _q(t, dtype):
    return t.to(dtype).float()


# ---------------------------------------------------------------- the processor
def smooth_image(H, W, seed):
    """The generator's test image, restated: per channel 128 + three low-frequency 2-D cosines (frequencies <= 3 periods over the image,
    seeded phases, amplitudes 20 .. 45), plus uniform noise of +-6 levels; rounded and clipped to uint8."""
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
    """The arithmetic definition of emo_image_preprocess (include/emo_hip.h), CPU f32."""
    from emote_hack_amd.clip_vision import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, center_crop_offsets, resize_output_size
    H, W, _ = img_u8.shape
    rh, rw = resize_output_size(H, W, shortest_edge)
    top, left = center_crop_offsets(rh, rw, crop)
    x = img_u8.permute(2, 0, 1)[None].float()
    y = torch.nn.functional.interpolate(x, size=(rh, rw), mode="bicubic", antialias=True, align_corners=False)
    y = y[0, :, top:top + crop, left:left + crop].clamp(0, 255) * (1.0 / 255.0)
    return (y - torch.tensor(OPENAI_CLIP_MEAN)[:, None, None]) / torch.tensor(OPENAI_CLIP_STD)[:, None, None]


def test_preprocess_vs_torch_definition():
    """emo_image_preprocess on the five seeded images (square, landscape, portrait, enlarging, identity) and on a random-noise frame
    (every tap matters) == F.interpolate(bicubic, antialias) + crop + clamp + rescale + normalise on the CPU."""
    from emote_hack_amd.clip_vision import CLIPImageProcessor
    proc = CLIPImageProcessor(device=DEV)
    seed = _meta()["proc_seed"]
    imgs = [smooth_image(H, W, seed + i) for i, (H, W) in enumerate(PROC_SIZES)]
    imgs.append(torch.randint(0, 256, (225, 301, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8))
    for img in imgs:
        got = proc(img.numpy(), return_tensors="pt").pixel_values
        assert got.shape == (1, 3, 224, 224) and got.dtype == torch.float32 and got.is_cuda
        ref = definition_pixels(img)
        print(f"preprocess {tuple(img.shape[:2])}: max |hip - definition| {float((got[0].cpu() - ref).abs().max()):.3e}")
        torch.testing.assert_close(got[0].cpu(), ref, rtol=RTOL, atol=ATOL)
        if tuple(img.shape[:2]) == (224, 224):
            # identity geometry: the taps are exactly (0, 1, 0, 0), so what is left is rescale, subtract, divide, each rounded to f32
            # on both sides (no fma across the first two) - the same bits
            assert torch.equal(got[0].cpu(), ref)
    # a list of mixed geometries and an (n, H, W, 3) batch come back in input order
    both = proc([imgs[0], imgs[1], imgs[1]]).pixel_values
    assert both.shape == (3, 3, 224, 224)
    torch.testing.assert_close(both[2].cpu(), definition_pixels(imgs[1]), rtol=RTOL, atol=ATOL)
    batch = proc(torch.stack([imgs[3], imgs[3].flip(0)])).pixel_values
    torch.testing.assert_close(batch[1].cpu(), definition_pixels(imgs[3].flip(0)), rtol=RTOL, atol=ATOL)
    assert torch.equal(batch[0], proc(imgs[3]).pixel_values[0])


def test_preprocess_vs_transformers_pil_processor(gold):
    """... and against the stored samples (every 4th row / column) of what transformers' PIL-backed CLIPImageProcessor returns.  PIL
    rounds to uint8 between its two passes, so it is not the arithmetic target: the bound per image is the recorded (definition vs PIL)
    max + atol, the mean within 1.25x the recorded mean."""
    from emote_hack_amd.clip_vision import CLIPImageProcessor
    meta = _meta()
    proc = CLIPImageProcessor(device=DEV)
    for i, (H, W) in enumerate(PROC_SIZES):
        got = proc(smooth_image(H, W, meta["proc_seed"] + i)).pixel_values[0].cpu()[:, ::4, ::4]
        rec = meta["processor_definition_vs_pil"][f"{H}x{W}"]
        e = (got - gold[f"proc/{H}x{W}"]).abs()
        print(f"preprocess {H}x{W} vs PIL: max {float(e.max()):.3e} (recorded {rec['max']:.3e}) mean {float(e.mean()):.3e} (recorded {rec['mean']:.3e})")
        assert float(e.max()) <= rec["max"] + ATOL and float(e.mean()) <= 1.25 * rec["mean"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,P", [(42, 14), (224, 14), (32, 8)])
def test_patch_rows(S, P, dtype):
    """bit-equal to unfold-style indexing rounded once to the dtype; columns (c, py, px); pad columns zero (K = 588 -> ld 592)"""
    from emote_hack_amd import ops
    B, G, K = 2, S // P, 3 * P * P
    pix = seeded_randn((B, 3, S, S), 31)
    got = ops.patch_rows(pix.to(DEV), P, dtype).cpu()
    ld = (K + 7) // 8 * 8
    assert got.shape == (B * G * G, ld) and got.dtype == dtype
    ref = pix.reshape(B, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, K).to(dtype)
    assert torch.equal(got[:, :K], ref)
    assert ld == K or bool((got[:, K:] == 0).all())
    # the same columns as F.unfold's
    unf = torch.nn.functional.unfold(pix, kernel_size=P, stride=P).transpose(1, 2).reshape(B * G * G, K)
    assert torch.equal(ref, unf.to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Np,Cc", [(9, 64), (256, 1024), (5, 40)])
def test_vision_embed(Np, Cc, dtype):
    """[class | patch rows] + position embedding, then LayerNorm == torch on the assembled tokens (inputs in the dtype, math in f32)"""
    from emote_hack_amd import ops
    B = 3
    patch, cls, pos = _q(seeded_randn((B * Np, Cc), 41), dtype), _q(seeded_randn((Cc,), 42), dtype), _q(seeded_randn((Np + 1, Cc), 43), dtype)
    g, b = 1 + 0.1 * seeded_randn((Cc,), 44), 0.1 * seeded_randn((Cc,), 45)
    got = ops.vision_embed(patch.to(DEV).to(dtype), cls.to(DEV).to(dtype), pos.to(DEV).to(dtype), g.to(DEV), b.to(DEV), B, 1e-5)
    assert got.shape == (B * (Np + 1), Cc) and got.dtype == dtype
    tok = torch.cat([cls.expand(B, 1, Cc), patch.view(B, Np, Cc)], 1) + pos[None]
    ref = torch.nn.functional.layer_norm(tok, (Cc,), g, b, 1e-5).reshape(-1, Cc)
    torch.testing.assert_close(got.float().cpu(), ref, **TOL[dtype])
    # a strided view of a wider buffer as the patch rows
    wide = torch.zeros(B * Np, Cc + 8, dtype=dtype, device=DEV)
    wide[:, :Cc] = patch.to(DEV).to(dtype)
    assert torch.equal(ops.vision_embed(wide[:, :Cc], cls.to(DEV).to(dtype), pos.to(DEV).to(dtype), g.to(DEV), b.to(DEV), B, 1e-5), got)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 16])
@pytest.mark.parametrize("L", [257, 10])
def test_noncausal_attention_at_the_encoder_shapes(L, d, dtype):
    """ops.attention without a mask at Lq = Lk = 257 (ViT-L/14, V^T ld 264) and 10 (the tiny tower), d = 64 and 16, against an f32 softmax"""
    from emote_hack_amd import ops
    B, heads = 2, 4
    C_ = heads * d
    qq, kk, vv = (_q(seeded_randn((B, L, C_), 50 + i), dtype) for i in range(3))
    ld = (L + 7) // 8 * 8
    vt = torch.full((B, C_, ld), float("nan"))            # pad columns must never be read into a result
    vt[:, :, :L] = vv.permute(0, 2, 1)
    got = ops.attention(qq.reshape(-1, C_).to(DEV).to(dtype), kk.reshape(-1, C_).to(DEV).to(dtype), vt.to(DEV).to(dtype), L, B=B, Lq=L,
                        heads=heads, d=d, scale=d ** -0.5)
    sp = lambda t: t.reshape(B, L, heads, d).permute(0, 2, 1, 3)
    s = torch.matmul(sp(qq), sp(kk).transpose(-1, -2)) * d ** -0.5
    ref = torch.matmul(s.softmax(-1), sp(vv)).permute(0, 2, 1, 3).reshape(B * L, C_)
    torch.testing.assert_close(got.float().cpu(), ref, **TOL[dtype])


# ---------------------------------------------------------------- the model against transformers' own
_MODELS = {}


def _pixels(name):
    m = _meta()
    S = m["configs"][name]["image_size"]
    return seeded_randn((2, 3, S, S), m["pixel_seed"][name])


def _model(name, dtype, projection=True):
    from emote_hack_amd.clip_vision import CLIPVisionModel, CLIPVisionModelWithProjection, clip_vision_synth_state_dict
    key = (name, dtype, projection)
    if key not in _MODELS:
        cfg = _meta()["configs"][name]
        m = (CLIPVisionModelWithProjection if projection else CLIPVisionModel)(cfg)
        m.load_state_dict(clip_vision_synth_state_dict(cfg))
        _MODELS[key] = m.to(DEV, dtype)
    return _MODELS[key]


def _lowp_check(tag, got, ref, yard, dtype):
    e = (got.float().cpu() - ref).abs()
    print(f"clip_vision {tag} {dtype}: mean err {float(e.mean()):.3e} max {float(e.max()):.3e} (transformers' own: mean {yard['mean']:.3e} max {yard['max']:.3e})")
    assert float(e.mean()) <= 2 * yard["mean"] and float(e.max()) <= 2.5 * yard["max"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_vs_transformers_golden(gold, dtype):
    """2 layers, 64 wide, 4 heads of 16, image 42 / patch 14 (10 tokens, K = 588 padded to 592), projection 32: every output and every
    hidden state; the output surface of both classes."""
    x = _pixels("tiny")
    out = _model("tiny", dtype)(x.to(DEV), output_hidden_states=True)
    assert out[0] is out.image_embeds and out[1] is out.last_hidden_state and out[2] is out.hidden_states
    assert out.image_embeds.shape == (2, 32) and out.last_hidden_state.shape == (2, 10, 64) and out.pooler_output.shape == (2, 64)
    assert len(out.hidden_states) == 3 and out.hidden_states[-1] is not None
    assert all(t.dtype == dtype for t in (out.image_embeds, out.last_hidden_state, out.pooler_output, *out.hidden_states))
    assert torch.equal(out.hidden_states[-1], out.last_hidden_state)
    plain = _model("tiny", dtype)(x)                                          # CPU pixel_values are uploaded; no hidden states unless asked
    assert plain.hidden_states is None and torch.equal(plain.image_embeds, out.image_embeds)
    with pytest.raises(IndexError):
        plain[2]
    bare = _model("tiny", dtype, projection=False)(x.to(DEV))
    assert bare[0] is bare.last_hidden_state and bare[1] is bare.pooler_output and not hasattr(bare, "image_embeds")
    assert torch.equal(bare.last_hidden_state, out.last_hidden_state) and torch.equal(bare.pooler_output, out.pooler_output)
    named = {"last_hidden_state": out.last_hidden_state, "pooler_output": out.pooler_output, "image_embeds": out.image_embeds,
             **{f"hidden_states.{i}": h for i, h in enumerate(out.hidden_states)}}
    if dtype == torch.float32:
        for k, t in named.items():
            torch.testing.assert_close(t.cpu(), gold[f"tiny/{k}"], rtol=RTOL, atol=ATOL, msg=lambda s, k=k: f"{k}: {s}")
    else:
        yard = _meta()["low_precision_error"]["tiny"][str(dtype).replace("torch.", "")]
        for k, t in named.items():
            _lowp_check("tiny " + k, t, gold[f"tiny/{k}"], yard["image_embeds" if k == "image_embeds" else "last_hidden_state"], dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_vitl14_vs_transformers_golden(gold, dtype):
    """The ViT-L/14 tower (24 layers of 16 heads x 64, 257 tokens, projection 768), B = 2: image_embeds, pooler_output, and every 8th
    token row of last_hidden_state and of hidden_states[-2]; outputs come back in the model's dtype."""
    out = _model("vitl14", dtype)(_pixels("vitl14").to(DEV), output_hidden_states=True)
    assert out.image_embeds.shape == (2, 768) and out.last_hidden_state.shape == (2, 257, 1024) and out.pooler_output.shape == (2, 1024)
    assert len(out.hidden_states) == 25 and out[0] is out.image_embeds
    assert all(t.dtype == dtype for t in (out.image_embeds, out.last_hidden_state, out.pooler_output, out.hidden_states[-2]))
    named = {"image_embeds": out.image_embeds, "pooler_output": out.pooler_output, "last_hidden_state_rows8": out.last_hidden_state[:, ::8],
             "hidden_states_m2_rows8": out.hidden_states[-2][:, ::8]}
    if dtype == torch.float32:
        for k, t in named.items():
            torch.testing.assert_close(t.cpu(), gold[f"vitl14/{k}"], rtol=RTOL, atol=ATOL, msg=lambda s, k=k: f"{k}: {s}")
    else:
        yard = _meta()["low_precision_error"]["vitl14"][str(dtype).replace("torch.", "")]
        for k, t in named.items():
            _lowp_check("vitl14 " + k, t, gold[f"vitl14/{k}"], yard["image_embeds" if k == "image_embeds" else "last_hidden_state"], dtype)


# ---------------------------------------------------------------- end to end
def _tiny_encoder(dtype=torch.float32):
    """the golden's tiny tower: projection_dim 32 = the cross-attention width of the tiny UNets (cases.TINY, cases.VIDEONET_TINY)"""
    return _model("tiny", dtype)


def test_pipeline_by_clip_image():
    """`pipeline("", clip_image=img)` with the HIP image encoder == the same call with text_embeddings= from _encode_image, bit for bit
    (a ONE-token context through context_kv / emo_attention); a second image on the reused plan differs from the first and equals a
    fresh pipeline's call."""
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    from emote_hack_amd.spec import param_shapes
    from emote_hack_amd.unet import UNet3DConditionModel

    def build(cfg, prefix="", cls=UNet3DConditionModel, **kw):
        m = cls(**cfg, **kw)
        m.load_state_dict(synth_state_dict(param_shapes(m.spec), prefix=prefix))
        return m.to(DEV, torch.float32)

    ref = build(cases.TINY, cases.REF_PREFIX, cls=AppearanceEncoderModel, _has_out=False)
    unet = build(cases.TINY_MOTION)
    enc = _tiny_encoder()

    def pipe():
        return EMOAnimationPipeline(unet=unet, scheduler=DDIMScheduler(), image_encoder=enc)

    img, img2 = smooth_image(60, 80, 3), smooth_image(96, 64, 4)
    lat, refl = seeded_randn((1, 4, 8, 16, 16), 5), seeded_randn((1, 4, 16, 16), 3)
    base = dict(video_length=8, height=128, width=128, output_type="latent", appearance_encoder=ref, seed=0, num_inference_steps=3,
                guidance_scale=7.5, context_frames=4, context_stride=1, context_overlap=2, ref_image_latents=refl)
    kw = lambda: dict(base, latents=lat.to(DEV))
    p = pipe()
    assert p.image_processor.size == {"shortest_edge": 42}
    out = p("", clip_image=img, **kw()).videos
    ctx = p._encode_image(img, DEV, 1, True)
    assert ctx.shape == (2, 1, 32) and not bool(ctx[0].any()) and bool(ctx[1].any())
    assert torch.equal(ctx[1:], p._encode_image(img, DEV, 1, False))
    assert torch.equal(ctx, p._encode_image(p.image_processor(img).pixel_values, DEV, 1, True))       # pixel_values handed over directly
    want = pipe()("", text_embeddings=ctx, **kw()).videos
    assert torch.equal(out, want)
    st = p._plan_cache[1]
    out2 = p("", clip_image=img2, **kw()).videos
    assert p._plan_cache[1] is st
    assert not torch.equal(out2, out)
    fresh = pipe()("", clip_image=img2, **kw()).videos
    assert torch.equal(out2, fresh)
    with pytest.raises(ValueError, match="prompt"):
        p("a cat", clip_image=img, **kw())


def test_videonet_with_image_embeds_vs_oracle():
    """VideoNet.forward(..., clip_condition_embeddings=image_embeds[:, None]) (models/videonet.py:255): two clips of four frames, each
    clip conditioned on its own image's embedding from the HIP encoder, against oracle.videonet_ref on the SAME embeddings."""
    from emote_hack_amd.spec import param_shapes
    from emote_hack_amd.videonet import VideoNet
    from oracle import videonet_ref as V
    vn = VideoNet(cases.VIDEONET_TINY, num_frames=4)
    sd = synth_state_dict(param_shapes(vn.spec), prefix="videonet.")
    vn.load_state_dict({"unet." + k: v for k, v in sd.items()})
    vn.to(DEV, torch.float32)
    emb = _tiny_encoder()(_pixels("tiny").to(DEV)).image_embeds                       # (2, 32)
    ctx = emb.repeat_interleave(4, dim=0)[:, None]                                    # (b t, 1, 32)
    assert ctx.shape == (8, 1, 32)
    bt, T = 8, 4
    noise = seeded_randn((bt, 4, 16, 16), 90)
    t = torch.tensor([961, 961, 961, 961, 500, 500, 500, 500])
    geo = {"down_blocks.0": (64, 16), "down_blocks.1": (64, 8), "down_blocks.2": (128, 4), "mid_block": (128, 2),
           "up_blocks.1": (128, 4), "up_blocks.2": (64, 8), "up_blocks.3": (64, 16)}
    refs = [seeded_randn((bt, *[(c, hw, hw) for k, (c, hw) in geo.items() if h.slot.startswith(k + ".")][0]), 100 + i)
            for i, h in enumerate(vn.ref_cond_attn_blocks)]
    with torch.no_grad():
        want = V.videonet_forward(sd, cases.VIDEONET_TINY, noise, t, refs, ctx.float().cpu(), T)
        other = V.videonet_forward(sd, cases.VIDEONET_TINY, noise, t, refs, ctx.float().cpu().flip(0), T)
    got = vn(noise.to(DEV), t.to(DEV), [r.to(DEV) for r in refs], ctx)
    assert got.shape == (bt, 4, 16, 16)
    torch.testing.assert_close(got.float().cpu(), want, rtol=RTOL, atol=ATOL)
    assert float((want - other).abs().max()) > 1e-3          # the one-token context is live: the other clip's image changes the result
