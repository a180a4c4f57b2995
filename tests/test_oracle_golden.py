"""Pin the oracle (oracle/*) against golden vectors captured from the reference's own code
(tools/oracle/gen_golden.py).  CPU only.  Tolerance: rtol 1e-3 / atol 1e-4 (north_star) - the
oracle actually matches to ~1e-6; integer paths are bit-exact."""
import json
import math
import os

import pytest
import torch
from safetensors.torch import load_file

from emote_hack_amd.synth import seeded_randn, synth_state_dict
from oracle import conditioning_ref as C
from oracle import scheduler_ref as S
from oracle import unet_ref as U
from oracle.pipeline_ref import denoise_loop
from tests import cases
from tests.block_cases import motion_shapes, resnet_shapes, tf_shapes  # noqa: F401  (the shape helpers live beside the block tables)

G = cases.GOLDEN_DIR
RTOL, ATOL = 1e-3, 1e-4


def close(a, b, rtol=RTOL, atol=ATOL):
    assert a.shape == b.shape, (a.shape, b.shape)
    torch.testing.assert_close(a, b, rtol=rtol, atol=atol)


@pytest.fixture(scope="module")
def ints():
    return json.load(open(os.path.join(G, "ints.json")))


@pytest.fixture(scope="module")
def mods():
    return load_file(os.path.join(G, "modules.safetensors"))


@pytest.fixture(scope="module")
def tiny():
    return load_file(os.path.join(G, "unet_tiny.safetensors"))


def sd_for(shapes, prefix):
    return synth_state_dict(shapes, prefix=prefix)


# ------------------------------------------------------------------ INT, bit-exact
def test_windows_bit_exact(ints):
    for c in ints["windows"]:
        f, ctx, stride, ov = c["args"]
        assert S.uniform_windows(0, 50, f, ctx, stride, ov) == c["windows"]
    for c in ints["windows_step"]:
        f, ctx, stride, ov = c["args"]
        assert S.uniform_windows(c["step"], 50, f, ctx, stride, ov) == c["windows"]


def test_speed_buckets_bit_exact(ints):
    sp = torch.tensor(ints["speed_buckets"]["speeds"])
    assert C.speed_bucket_index(sp).tolist() == ints["speed_buckets"]["buckets"]
    # survey probe goldens
    assert C.speed_bucket_index(torch.tensor([-1, -0.13, 0, 0.07, 0.49, 2.0])).tolist() == [0, 3, 4, 4, 6, 8]


def test_timestep_tables():
    assert S.timestep_table(50, 1000, 0) == list(range(980, -1, -20))
    assert S.timestep_table(50, 1000, 1) == list(range(981, 0, -20))


def test_bank_order(ints):
    strip = lambda names: [n.replace(".transformer_blocks.0", "") for n in names]
    assert U.transformer_block_order(cases.TINY_MOTION, "midup") == strip(ints["bank_order_tiny_midup"])
    assert U.transformer_block_order(cases.TINY_MOTION, "full") == strip(ints["bank_order_tiny_full"])
    assert U.transformer_block_order(cases.SD15_MOTION, "midup") == strip(ints["bank_order_sd15_midup"])


# ------------------------------------------------------------------ modules
def test_timestep_embedding(mods):
    ts = torch.tensor([981, 1, 500, 0, 999])
    e = U.timestep_embedding(ts, 320, True, 0)
    g = mods["temb/sinusoid320"]
    # fp32 exp of the frequencies may differ in the last bit from one CPU to another (same torch build): with the rounding of
    # the product, the angle t * freq is known to |angle| * 2^-22 and so are its sin / cos (observed: 2.9e-5 at t = 999);
    # on top of that, rtol 1e-5 / atol 1e-6
    ang = (ts[:, None].float() * torch.exp(-math.log(10000) * torch.arange(160, dtype=torch.float32) / 160)[None, :]).abs()
    tol = 1e-6 + 1e-5 * g.abs() + torch.cat([ang, ang], -1) * 2.0 ** -22
    assert e.shape == g.shape and ((e - g).abs() <= tol).all(), float(((e - g).abs() - tol).max())
    # survey probe golden
    assert torch.allclose(e[0, :3], torch.tensor([0.67996, -0.79843, 0.57806]), atol=1e-4)
    assert torch.allclose(e[0, 160:163], torch.tensor([0.73325, 0.60209, 0.81599]), atol=1e-4)
    close(U.timestep_embedding(ts, 32, False, 1), mods["temb/sinusoid32_noflip_shift1"], 1e-5, 1e-6)
    sd = sd_for({"linear_1.weight": (128, 32), "linear_1.bias": (128,), "linear_2.weight": (128, 128),
                 "linear_2.bias": (128,)}, "time_embedding.")
    t = U.timestep_embedding(ts, 32, True, 0)
    out = U._lin(sd, "linear_2", torch.nn.functional.silu(U._lin(sd, "linear_1", t)))
    close(out, mods["temb/mlp_out"])


@pytest.mark.parametrize("name,cin,cout", [("resnet_sc", 32, 64), ("resnet_id", 64, 64)])
def test_resnet(mods, name, cin, cout):
    sd = {"r." + k: v for k, v in sd_for(resnet_shapes(cin, cout), name + ".").items()}
    x, emb = seeded_randn((2, cin, 4, 8, 8), 11), seeded_randn((2, 128), 12)
    close(U.resnet_block(sd, "r", x, emb, 8, 1e-5), mods[f"{name}/out"])


def test_samplers(mods):
    sd = {"d." + k: v for k, v in sd_for({"conv.weight": (64, 64, 3, 3), "conv.bias": (64,)}, "down.").items()}
    close(U._conv_per_frame(sd, "d.conv", seeded_randn((1, 64, 3, 8, 8), 13), stride=2, padding=1), mods["down/out"])
    sd = {"u." + k: v for k, v in sd_for({"conv.weight": (64, 64, 3, 3), "conv.bias": (64,)}, "up.").items()}
    close(U.upsample(sd, "u", seeded_randn((1, 64, 3, 4, 4), 14)), mods["up/out"])


def attn_shapes(c, kv):
    return {"to_q.weight": (c, c), "to_k.weight": (c, kv), "to_v.weight": (c, kv), "to_out.0.weight": (c, c),
            "to_out.0.bias": (c,)}


@pytest.mark.parametrize("d", [40, 80, 160])
def test_attention_real_head_dims(mods, d):
    c = 8 * d
    sd = {"a." + k: v for k, v in sd_for(attn_shapes(c, c), f"attn{d}.").items()}
    x = seeded_randn((1, 64, c), 20 + d)
    close(U.attention(sd, "a", x, None, 8), mods[f"attn{d}/self_out"])
    sd = {"a." + k: v for k, v in sd_for(attn_shapes(c, 768), f"xattn{d}.").items()}
    close(U.attention(sd, "a", x, seeded_randn((1, 7, 768), 21 + d), 8), mods[f"attn{d}/cross_out"])


def test_feed_forward(mods):
    sd = {"f." + k: v for k, v in sd_for({"net.0.proj.weight": (512, 64), "net.0.proj.bias": (512,),
                                          "net.2.weight": (64, 256), "net.2.bias": (64,)}, "ff.").items()}
    close(U.feed_forward(sd, "f", seeded_randn((2, 16, 64), 30)), mods["ff/out"])


@pytest.mark.parametrize("name,lin", [("tf3d", False), ("tf3d_lin", True)])
def test_transformer3d(mods, name, lin):
    sd = {"t." + k: v for k, v in sd_for(tf_shapes(64, 32, lin), name + ".").items()}
    x = seeded_randn((2, 64, 3, 4, 4), 40)
    close(U.transformer3d(sd, "t", x, seeded_randn((2, 5, 32), 41), 4, 8, lin), mods[f"{name}/out"])
    close(U.transformer3d(sd, "t", x, seeded_randn((6, 5, 32), 42), 4, 8, lin), mods[f"{name}/out_perframe_ctx"])


def test_motion_module(mods):
    sd = {"m." + k: v for k, v in sd_for(motion_shapes(64, 4), "motion.").items()}
    close(U.motion_module(sd, "m", seeded_randn((2, 64, 4, 4, 4), 50), 4), mods["motion/out"])
    sd = {"m." + k: v for k, v in sd_for(motion_shapes(320, 8), "motion320.").items()}
    close(U.motion_module(sd, "m", seeded_randn((1, 320, 12, 4, 4), 51), 8), mods["motion320/out"])


# ------------------------------------------------------------------ tiny UNet end to end
def tiny_sd(cfg, prefix="", has_out=True):
    from emote_hack_amd.spec import build_spec, param_shapes
    return synth_state_dict(param_shapes(build_spec(cfg, has_out=has_out)), prefix=prefix)


def test_unet_tiny_plain_motion_linear(tiny):
    x, ctx = cases.tiny_inputs(2, 4)
    close(U.unet_forward(tiny_sd(cases.TINY), cases.TINY, x[:, :, :2], 981, ctx), tiny["plain/out"])
    sd = tiny_sd(cases.TINY_MOTION)
    close(U.unet_forward(sd, cases.TINY_MOTION, x, torch.tensor(961), ctx), tiny["motion/out"])
    close(U.unet_forward(tiny_sd(cases.TINY_LINEAR), cases.TINY_LINEAR, x, 500, ctx), tiny["linear/out"])


def ctrl_residuals():
    res_shapes = [(2, 32, 4, 16, 16)] * 3 + [(2, 32, 4, 8, 8)] + [(2, 64, 4, 8, 8)] * 2 + [(2, 64, 4, 4, 4)] * 3 + \
                 [(2, 64, 4, 2, 2)] * 3
    return tuple(0.1 * seeded_randn(s, 100 + i) for i, s in enumerate(res_shapes)), 0.1 * seeded_randn((2, 64, 4, 2, 2), 99)


def test_unet_tiny_controlnet_residuals(tiny):
    x, ctx = cases.tiny_inputs(2, 4)
    down_res, mid_res = ctrl_residuals()
    y = U.unet_forward(tiny_sd(cases.TINY_MOTION), cases.TINY_MOTION, x, 961, ctx,
                       down_block_additional_residuals=down_res, mid_block_additional_residual=mid_res)
    close(y, tiny["motion/out_ctrl"])


def test_reference_write_read(tiny):
    x, ctx = cases.tiny_inputs(2, 4)
    ref_sd = tiny_sd(cases.TINY, cases.REF_PREFIX)
    ref_lat = seeded_randn((1, 4, 16, 16), 3).repeat(2, 1, 1, 1).unsqueeze(2)
    _, written = U.unet_forward(ref_sd, cases.TINY, ref_lat, 961, ctx, bank_mode="write")
    order = U.transformer_block_order(cases.TINY, "midup")
    assert len(order) == 10
    for i, p in enumerate(order):
        close(written[p], tiny[f"banks/{i}"])
    banks = U.round_banks_fp16(written)
    y = U.unet_forward(tiny_sd(cases.TINY_MOTION), cases.TINY_MOTION, x, 961, ctx, bank_mode="read", banks=banks,
                       uc_rows=cases.uc_rows(2, 4))
    close(y, tiny["read/out"])
    # uc rows must equal a run without banks (SURVEY 3.3 probe)
    close(y[:1], tiny["motion/out"][:1], 1e-4, 1e-5)
    assert (y[1] - tiny["motion/out"][1]).abs().max() > 1e-2


def test_reference_write_read_fusion_blocks_full(tiny):
    """fusion_blocks="full" (mutual_self_attention.py:532-537): all 16 transformer blocks write / read, down path included."""
    x, ctx = cases.tiny_inputs(2, 4)
    ref_lat = seeded_randn((1, 4, 16, 16), 3).repeat(2, 1, 1, 1).unsqueeze(2)
    _, written = U.unet_forward(tiny_sd(cases.TINY, cases.REF_PREFIX), cases.TINY, ref_lat, 961, ctx, bank_mode="write", fusion_blocks="full")
    order = U.transformer_block_order(cases.TINY, "full")
    assert len(order) == 16
    for i, p in enumerate(order):
        close(written[p], tiny[f"banks_full/{i}"])
    y = U.unet_forward(tiny_sd(cases.TINY_MOTION), cases.TINY_MOTION, x, 961, ctx, bank_mode="read", banks=U.round_banks_fp16(written),
                       uc_rows=cases.uc_rows(2, 4), fusion_blocks="full")
    close(y, tiny["read/out_full"])
    assert (y[1] - tiny["read/out"][1]).abs().max() > 1e-2


# (prefix of tests/golden/loop_tiny.safetensors, scheduler, context_batch_size, guidance_scale): ddim_cbs2 = three windows in a
# full + a partial batch with the reference's literal text / bank-row pairing at cbs > 1; ddim_nocfg = guidance_scale 1.0
LOOP_CASES = [("ddim", "ddim", 1, 7.5), ("ddpm", "ddpm", 1, 7.5), ("ddim_cbs2", "ddim", 2, 7.5), ("ddim_nocfg", "ddim", 1, 1.0)]


@pytest.mark.parametrize("prefix,kind,cbs,gs", LOOP_CASES)
def test_denoise_loop(prefix, kind, cbs, gs):
    g = load_file(os.path.join(G, "loop_tiny.safetensors"))
    lat, eps = denoise_loop(tiny_sd(cases.TINY_MOTION), cases.TINY_MOTION, tiny_sd(cases.TINY, cases.REF_PREFIX),
                            cases.TINY, seeded_randn((1, 4, 8, 16, 16), 5), seeded_randn((1, 4, 16, 16), 3),
                            seeded_randn((2, 5, 32), 2), scheduler=S.SchedulerRef(kind), num_inference_steps=3,
                            guidance_scale=gs, context_frames=4, context_stride=1, context_overlap=2, seed=0,
                            return_eps=True, context_batch_size=cbs)
    for i in range(3):
        close(eps[i], g[f"{prefix}/eps{i}"], 1e-3, 1e-4)  # measured worst 0.68 of the bound (profiles/r02f_loop_error.txt holds the HIP side)
    close(lat, g[f"{prefix}/latents"], 1e-3, 1e-4)


# ------------------------------------------------------------------ scheduler self-consistency (parity unpinned)
@pytest.mark.parametrize("kind", ["ddim", "ddpm"])
def test_scheduler_coefficients_match_step(kind):
    sch = S.SchedulerRef(kind)
    ts = sch.set_timesteps(50)
    x, eps, z = seeded_randn((1, 4, 2, 8, 8), 1), seeded_randn((1, 4, 2, 8, 8), 2), seeded_randn((1, 4, 2, 8, 8), 3)
    for t in (ts[0], ts[10], ts[-2], ts[-1]):
        cx, ce, cn = sch.coefficients(t)
        close(cx * x + ce * eps + cn * z, sch.step(eps, t, x, noise=z), 1e-5, 1e-5)


def test_ddim_x0_identity():
    """EMOAnimationPipeline.py:397-399: pred_x0 = (x - sqrt(1-a) eps)/sqrt(a); a DDIM step with the
    TRUE eps walks x_t = sqrt(a)x0 + sqrt(1-a)eps to the same x0 at the previous alpha."""
    sch = S.SchedulerRef("ddim")
    ts = sch.set_timesteps(50)
    x0, eps = seeded_randn((1, 4, 1, 8, 8), 1), seeded_randn((1, 4, 1, 8, 8), 2)
    t = ts[5]
    a, ap = sch.alphas_cumprod[t], sch.alphas_cumprod[t - 20]
    xt = a.sqrt() * x0 + (1 - a).sqrt() * eps
    close(sch.step(eps, t, xt), ap.sqrt() * x0 + (1 - ap).sqrt() * eps, 1e-4, 1e-5)


def test_counter_normal_stats():
    z = S.counter_normal(0, 3, 1 << 16)
    assert abs(float(z.mean())) < 0.02 and abs(float(z.std()) - 1) < 0.02
    assert torch.equal(z, S.counter_normal(0, 3, 1 << 16))
    assert not torch.equal(z, S.counter_normal(0, 4, 1 << 16))


# ------------------------------------------------------------------ conditioning (A17/A18)
def test_conditioning():
    g = load_file(os.path.join(G, "conditioning.safetensors"))
    sp = torch.tensor(cases.SPEEDS, dtype=torch.float32)
    close(C.speed_encoder_encode(sp), g["speed_encoder/encode"], 1e-5, 1e-6)
    # survey probe golden
    assert torch.allclose(C.speed_encoder_encode(torch.tensor([-0.13]))[0],
                          torch.tensor([1, 1, 0.9705, -0.7163, -0.9992, -1, -1, -1, -1.0]), atol=1e-4)
    sd = sd_for({"mlp.0.weight": (64, 9), "mlp.0.bias": (64,), "mlp.2.weight": (64, 64), "mlp.2.bias": (64,)}, "speed_encoder.")
    close(C.speed_encoder(sd, sp), g["speed_encoder/out"])
    sd = sd_for({"speed_embedding.weight": (9, 64), "speed_mlp.0.weight": (64, 64),
                 "speed_mlp.0.bias": (64,), "speed_mlp.2.weight": (64, 64), "speed_mlp.2.bias": (64,)}, "speed_controller.")
    close(C.speed_controller(sd, sp), g["speed_controller/out"])
    chans = [1, 64, 128, 256, 32]
    shp = {}
    for i, k in enumerate((0, 2, 4, 6)):
        shp[f"encoder.{k}.weight"] = (chans[i + 1], chans[i], 3, 3)
        shp[f"encoder.{k}.bias"] = (chans[i + 1],)
    close(C.face_region_controller(sd_for(shp, "face_region."), seeded_randn((2, 1, 8, 8), 60)), g["face_region/out"])
    lay = {}
    for i in range(2):
        for n in ("query", "key", "value"):
            lay[f"layers.{i}.{n}.weight"] = (48, 48)
            lay[f"layers.{i}.{n}.bias"] = (48,)
    close(C.net_audio_attention_layers(sd_for(lay, "audio_layers."), seeded_randn((2, 6, 48), 61),
                                       seeded_randn((2, 6, 48), 62), 2), g["audio_layers/out"])
    one = {f"{n}.{w}": ((48, 48) if w == "weight" else (48,)) for n in ("query", "key", "value") for w in ("weight", "bias")}
    close(C.net_reference_attention_layer(sd_for(one, "ref_layer."), seeded_randn((2, 6, 48), 63),
                                          seeded_randn((2, 1, 48), 64)), g["ref_layer/out"])
    sd = sd_for({"frame_proj.weight": (64, 64), "frame_proj.bias": (64,), "audio_proj.weight": (64, 768),
                 "audio_proj.bias": (64,), "out_proj.weight": (64, 64), "out_proj.bias": (64,)}, "stage2_audio.")
    close(C.stage2_audio_attention(sd, seeded_randn((2, 12, 64), 65), seeded_randn((2, 5, 768), 66)), g["stage2_audio/out"])
    sd = sd_for({"temperature": (8, 1, 1), "qkv.weight": (192, 64), "proj.weight": (64, 64), "proj.bias": (64,)}, "stage2_temporal.")
    close(C.stage2_temporal_attention(sd, seeded_randn((2, 12, 64), 67)), g["stage2_temporal/out"])


# ------------------------------------------------------------------ BASELINE config 1 (860 M params; ~1 min)
def test_cfg1_unet_config_yaml_shape():
    path = os.path.join(G, "cfg1.safetensors")
    if not os.path.exists(path):
        pytest.skip("cfg1 golden not generated")
    from emote_hack_amd.spec import build_spec, param_shapes
    cfg = dict(cases.SD15, norm_num_groups=4)  # configs/unet-config.yaml:default
    sd = synth_state_dict(param_shapes(build_spec(cfg)))
    y = U.unet_forward(sd, cfg, seeded_randn((1, 4, 1, 32, 32), 1), 981, seeded_randn((1, 77, 768), 2))
    close(y, load_file(path)["cfg1/out"])


def test_controlnet_cond_embedding_vs_reference():
    """oracle/controlnet_ref.cond_embedding vs the reference's ControlNetConditioningEmbedding (controlnet.py:49-91) run
    through tools/oracle/gen_golden.py (same synthesised weights by key name)."""
    from oracle.controlnet_ref import cond_embedding
    from emote_hack_amd.synth import synth_state_dict
    shapes = {"controlnet_cond_embedding.conv_in.weight": (16, 3, 3, 3), "controlnet_cond_embedding.conv_in.bias": (16,)}
    cc = (16, 32, 96, 256)
    for i in range(3):
        shapes[f"controlnet_cond_embedding.blocks.{2 * i}.weight"] = (cc[i], cc[i], 3, 3)
        shapes[f"controlnet_cond_embedding.blocks.{2 * i}.bias"] = (cc[i],)
        shapes[f"controlnet_cond_embedding.blocks.{2 * i + 1}.weight"] = (cc[i + 1], cc[i], 3, 3)
        shapes[f"controlnet_cond_embedding.blocks.{2 * i + 1}.bias"] = (cc[i + 1],)
    shapes["controlnet_cond_embedding.conv_out.weight"] = (32, 256, 3, 3)
    shapes["controlnet_cond_embedding.conv_out.bias"] = (32,)
    # gen_golden synthesises under the module-local names with the prefix as salt: same (prefix + local key) strings
    sd = synth_state_dict({k[len("controlnet_cond_embedding."):]: v for k, v in shapes.items()}, prefix="controlnet_cond_embedding.")
    sd = {"controlnet_cond_embedding." + k: v for k, v in sd.items()}
    g = load_file(os.path.join(G, "controlnet.safetensors"))
    y = cond_embedding(sd, seeded_randn((2, 3, 64, 64), 70))
    torch.testing.assert_close(y, g["cond_embedding/out"], rtol=1e-4, atol=1e-5)


def test_controlnet_state_dict_keys_follow_the_reference_module_tree():
    """Key names / shapes of ControlNetModel (controlnet.py:94-262): cond embedding, down blocks, 12 + 1 zero convs, mid."""
    from emote_hack_amd.spec import build_spec, param_shapes, skip_channels
    sp = build_spec(dict(cases.SD15, down_block_types=("CrossAttnDownBlock3D",) * 3 + ("DownBlock3D",)), controlnet=(16, 32, 96, 256))
    d = param_shapes(sp)
    assert skip_channels(sp) == [320, 320, 320, 320, 640, 640, 640, 1280, 1280, 1280, 1280, 1280]
    assert d["controlnet_cond_embedding.conv_in.weight"] == (16, 3, 3, 3)
    assert d["controlnet_cond_embedding.blocks.5.weight"] == (256, 96, 3, 3)
    assert d["controlnet_cond_embedding.conv_out.weight"] == (320, 256, 3, 3)
    assert d["controlnet_down_blocks.11.weight"] == (1280, 1280, 1, 1) and "controlnet_down_blocks.12.weight" not in d
    assert d["controlnet_mid_block.weight"] == (1280, 1280, 1, 1)
    assert not any(k.startswith(("up_blocks.", "conv_out.", "conv_norm_out.")) for k in d)
    assert "mid_block.attentions.0.transformer_blocks.0.attn1.to_q.weight" in d


def test_unet_non_multiple_of_8_input(tiny):
    """unet_controlnet.py:357-365,456-459: H / W not a multiple of 2^num_upsamplers -> the upsamplers interpolate to the skip
    tensor's size (20x12 -> 10x6 -> 5x3 -> 3x2 and back).  Golden from the reference's own UNet."""
    y = U.unet_forward(tiny_sd(cases.TINY_MOTION), cases.TINY_MOTION, seeded_randn((1, 4, 2, 20, 12), 1), 500, seeded_randn((1, 5, 32), 2))
    close(y, tiny["motion/out_20x12"])


def test_denoise_loop_wrapped_window_is_deterministic():
    """A wrapped window (context_stride 2) lists frames twice; the restatement pins the serial outcome of the reference's
    index assignment (EMOAnimationPipeline.py:792-794: last occurrence wins).  torch's own index_put races on duplicates once
    it goes multi-threaded (numel >= 32768 here), so: same result with 1 thread and with many, and equal to an explicit
    serial accumulation of the last occurrences."""
    args = (tiny_sd(cases.TINY_MOTION), cases.TINY_MOTION, tiny_sd(cases.TINY, cases.REF_PREFIX), cases.TINY,
            seeded_randn((1, 4, 20, 16, 16), 5), seeded_randn((1, 4, 16, 16), 3), seeded_randn((2, 5, 32), 2))
    kw = dict(scheduler=S.SchedulerRef("ddim"), num_inference_steps=1, guidance_scale=7.5, context_frames=16, context_stride=2,
              context_overlap=4, seed=0)
    n = torch.get_num_threads()
    try:
        torch.set_num_threads(1)
        a = denoise_loop(*args, **kw)
        torch.set_num_threads(max(n, 4))
        b = denoise_loop(*args, **kw)
    finally:
        torch.set_num_threads(n)
    close(a, b, 1e-5, 1e-6)   # thread count only changes the f32 summation order inside the GEMMs


# ----------------------------------------------------------------------------- wav2vec2 front-end
def test_wav2vec2_oracle_matches_transformers_goldens():
    """oracle/wav2vec2_ref.py against the outputs of transformers' own Wav2Vec2Model (the third-party class Net.py:607-612 loads;
    tools/oracle/gen_golden_wav2vec2.py): the 2-layer member of the base family, the full wav2vec2-base configuration on 1 s of
    audio (94 M name-keyed synthetic parameters, regenerated here), the utterance normalisation of its processor and the
    reference's own windowing (Net.py:646-667)."""
    from emote_hack_amd.wav2vec2 import wav2vec2_synth_state_dict
    from oracle import wav2vec2_ref as W
    g = load_file(os.path.join(cases.GOLDEN_DIR, "wav2vec2.safetensors"))
    with torch.no_grad():
        y = W.wav2vec2_forward(wav2vec2_synth_state_dict(cases.WAV2VEC2_TINY), cases.WAV2VEC2_TINY, 0.5 * seeded_randn((1, 4000), 501))
        torch.testing.assert_close(y, g["tiny/out"], rtol=1e-4, atol=1e-5)
        sd = wav2vec2_synth_state_dict({})
        wave = 0.1 * seeded_randn((16000,), 502) + 0.05 * torch.sin(torch.arange(16000) * 0.05)
        torch.testing.assert_close(W.normalize_waveform(wave.reshape(1, -1)), g["base/input_values"], rtol=1e-5, atol=1e-6)
        yb = W.wav2vec2_forward(sd, {}, g["base/input_values"])
        torch.testing.assert_close(yb, g["base/out"], rtol=1e-3, atol=1e-4)
        torch.testing.assert_close(W.audio_features(sd, {}, wave), g["base/features"], rtol=1e-3, atol=1e-4)
    assert float(g["base/out"].std()) > 0.5        # a live signal, not a constant


# ----------------------------------------------------------------------------- VideoNet (models/videonet.py)
def _rcab_sd():
    """weights of the golden's ReferenceConditionedAttentionBlock: name-keyed under the block's own key names, salt 'rcab.'"""
    from emote_hack_amd.spec import param_shapes
    from emote_hack_amd.unet import UNet3DConditionModel  # noqa: F401  (host-side structure walk only)
    from emote_hack_amd.videonet import VideoNet
    vn = VideoNet(cases.VIDEONET_TINY, num_frames=4)
    slot = "down_blocks.0.attentions.0."
    return synth_state_dict({k[len(slot):]: v for k, v in param_shapes(vn.spec).items() if k.startswith(slot)}, prefix="rcab.")


def test_videonet_oracle_matches_the_reference_classes():
    """oracle/videonet_ref.py against goldens produced by the reference's own class bodies (tools/oracle/gen_golden.py gen_videonet):
    SpatialAttentionModule, ReferenceConditionedAttentionBlock.forward (sam -> cross_attn -> tam, skip_temporal_attn, a changed
    num_frames), and VideoNet.__init__ / update_reference_embeddings (block order, dealing, key listing)."""
    from oracle import videonet_ref as V
    g = load_file(os.path.join(cases.GOLDEN_DIR, "videonet.safetensors"))
    sd = {"sam." + k: v for k, v in synth_state_dict({k[4:]: v for k, v in _sam_shapes(64).items()}, prefix="videonet_spatial.").items()}
    with torch.no_grad():
        y = V.spatial_attention_module(sd, "sam", seeded_randn((3, 64, 4, 8), 80), seeded_randn((3, 64, 4, 8), 81))
        torch.testing.assert_close(y, g["spatial/out"], rtol=1e-4, atol=1e-5)
        rsd = {"blk." + k: v for k, v in _rcab_sd().items()}
        x, r, ctx = seeded_randn((8, 64, 4, 8), 83), seeded_randn((8, 64, 4, 8), 84), seeded_randn((8, 5, 32), 85)
        torch.testing.assert_close(V.rcab(rsd, "blk", x, r, ctx, 8, 32, 4), g["rcab/out"], rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(V.rcab(rsd, "blk", x, r, ctx, 8, 32, 4, skip_temporal_attn=True), g["rcab/out_skip"], rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(V.rcab(rsd, "blk", x, r, ctx, 8, 32, 2), g["rcab/out_frames2"], rtol=1e-4, atol=1e-5)
    assert float((g["rcab/out"] - g["rcab/out_skip"]).abs().mean()) > 1e-2 and float((g["rcab/out"] - g["rcab/out_frames2"]).abs().mean()) > 1e-3
    wiring = json.load(open(os.path.join(cases.GOLDEN_DIR, "videonet_wiring.json")))
    assert V.block_order(cases.VIDEONET_TINY) == wiring["block_order"]
    assert wiring["reference_index_of_block"] == list(range(len(wiring["block_order"])))


def _sam_shapes(c):
    from emote_hack_amd.spec import _sam_shapes as shapes
    d = {}
    shapes("sam", c, d)
    return d


def test_videonet_state_dict_keys_and_block_order_match_the_reference_ctor():
    """The product VideoNet owns exactly the keys (and shapes) of the reference's VideoNet built on the same 2-D UNet, and deals the
    reference embeddings to its blocks in the reference's order (tests/golden/videonet_wiring.json)."""
    from emote_hack_amd.videonet import VideoNet
    wiring = json.load(open(os.path.join(cases.GOLDEN_DIR, "videonet_wiring.json")))
    vn = VideoNet(cases.VIDEONET_TINY, num_frames=4)
    assert {"unet." + k: list(v) for k, v in vn._shapes.items()} == {k: v for k, v in wiring["keys"]}
    assert [h.slot for h in vn.ref_cond_attn_blocks] == wiring["block_order"]
    refs = [torch.full((1,), float(i)) for i in range(len(vn.ref_cond_attn_blocks))]
    vn.update_reference_embeddings(refs)
    assert [int(b.reference_tensor.item()) for b in vn.ref_cond_attn_blocks] == wiring["reference_index_of_block"]
    with pytest.raises(ValueError, match="2-D UNet"):
        VideoNet(cases.TINY_MOTION)


# ----------------------------------------------------------------------------- Net.py placeholders
def test_net_placeholder_oracles_match_the_reference_classes():
    """oracle/conditioning_ref.py against the reference's own ReferenceAttention / MotionModule class bodies and the runnable stages of
    BackboneNetwork.forward (tests/golden/net_placeholders.safetensors); net_placeholders.json records what the reference RAISES for the
    geometries / classes that do not run (the product refuses the same ones)."""
    g = load_file(os.path.join(cases.GOLDEN_DIR, "net_placeholders.safetensors"))
    J = json.load(open(os.path.join(cases.GOLDEN_DIR, "net_placeholders.json")))
    assert J == {"motion_module_4x4": "RuntimeError", "motion_module_even_kernel": "RuntimeError", "temporal_module": "RuntimeError",
                 "backbone_forward": "AssertionError"}
    from emote_hack_amd.net_placeholders import MotionModule, ReferenceAttention
    with torch.no_grad():
        sd = synth_state_dict(ReferenceAttention(64)._shapes, prefix="net_reference_attention.")
        y = C.net_reference_attention(sd, seeded_randn((2, 64, 4, 6), 400), seeded_randn((2, 64, 4, 6), 401))
        torch.testing.assert_close(y, g["reference_attention/out"], rtol=1e-4, atol=1e-5)
        sd = synth_state_dict(MotionModule(64, 3)._shapes, prefix="net_motion_module.")
        torch.testing.assert_close(C.net_motion_module(sd, seeded_randn((2, 64, 6, 1, 1), 402)), g["motion_module/out"], rtol=1e-4, atol=1e-5)
        feat = 32
        shp = {f"{i}.{n}.{w}": ((feat, feat) if w == "weight" else (feat,)) for i in range(2) for n in ("query", "key", "value") for w in ("weight", "bias")}
        rsd = synth_state_dict(shp, prefix="net_backbone_ref.")
        asd = synth_state_dict({"layers." + k: v for k, v in shp.items()}, prefix="net_backbone_audio.")
        lat, aud, ref = seeded_randn((2, 5, feat), 405), seeded_randn((2, 5, feat), 406), seeded_randn((2, 1, feat), 407)
        x = lat
        for i in range(2):      # BackboneNetwork.forward :401-403 adds a SECOND skip around a layer that already has one
            x = C.net_reference_attention_layer({k[2:]: v for k, v in rsd.items() if k.startswith(f"{i}.")}, x, ref) + x
        torch.testing.assert_close(C.net_audio_attention_layers(asd, x, aud, 2), g["backbone/before_temporal"], rtol=1e-4, atol=1e-5)


# ----------------------------------------------------------------------------- UNet forward switches (unet_controlnet.py:371-373,400-408)
SWITCH_CASES = {"center": (dict(center_input_sample=True), None),
                "class_table": (dict(num_class_embeds=7), lambda: torch.tensor([3, 5])),
                "class_timestep": (dict(class_embed_type="timestep"), lambda: torch.tensor([10, 500])),
                "class_identity": (dict(class_embed_type="identity"), lambda: 0.1 * seeded_randn((2, 128), 71))}


@pytest.mark.parametrize("name", sorted(SWITCH_CASES))
def test_unet_forward_switches_oracle_vs_reference(name):
    """center_input_sample and the three class-embedding forms: the oracle against the reference model's own output."""
    from emote_hack_amd.spec import build_spec, param_shapes
    g = load_file(os.path.join(cases.GOLDEN_DIR, "unet_switches.safetensors"))
    extra, labels = SWITCH_CASES[name]
    cfg = dict(cases.TINY_MOTION, **extra)
    sd = synth_state_dict(param_shapes(build_spec(cfg)))
    x, ctx = cases.tiny_inputs(2, 4)
    with torch.no_grad():
        y = U.unet_forward(sd, cfg, x, 961, ctx, class_labels=labels() if labels else None)
    torch.testing.assert_close(y, g[name + "/out"], rtol=1e-4, atol=1e-5)
    if labels:
        with pytest.raises(ValueError, match="class_labels"):
            U.unet_forward(sd, cfg, x, 961, ctx)


def test_attention_mask_is_a_dead_input_of_the_reference_unet():
    """The reference forwards attention_mask to its blocks and the blocks drop it: the golden taken WITH a mask equals the plain forward's."""
    g = load_file(os.path.join(cases.GOLDEN_DIR, "unet_switches.safetensors"))
    tiny = load_file(os.path.join(cases.GOLDEN_DIR, "unet_tiny.safetensors"))
    assert torch.equal(g["attention_mask/out"], tiny["motion/out"])
