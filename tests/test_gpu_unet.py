"""GPU parity tests, model level: the HIP UNet / ReferenceNet / sampling loop vs (a) golden vectors
captured from the reference (tests/golden) and (b) the CPU oracle on seeded inputs.
f32 mode: rtol 1e-3 / atol 1e-4 (north_star).  bf16 / fp16 mode: vs the same fp32 goldens, bounded by the reference's
OWN error in that dtype on the same model and inputs (goldens motion/out_bf16 etc.: mean 8.7e-3 / max 4.8e-2 at
output mean-abs 0.47 in bf16, 1.1e-3 / 5.2e-3 in fp16)."""
import os

import pytest
import torch
from safetensors.torch import load_file

from emote_hack_amd.synth import seeded_randn, synth_state_dict
from tests import cases

pytestmark = pytest.mark.gpu
G = cases.GOLDEN_DIR
DEV = "cuda"


def build(cfg, dtype, prefix="", cls=None, has_out=True):
    from emote_hack_amd.unet import UNet3DConditionModel
    from emote_hack_amd.spec import build_spec, param_shapes
    cls = cls or UNet3DConditionModel
    m = cls(**cfg) if has_out else cls(**cfg, _has_out=False)
    sd = synth_state_dict(param_shapes(m.spec), prefix=prefix)
    m.load_state_dict(sd)
    return m.to(DEV, dtype)


_YARD = {}


def yardstick(dtype):
    """The reference's OWN low-precision error on the tiny motion UNet (tests/golden/unet_tiny.safetensors motion/out_bf16 and
    motion/out_fp16: the reference model run in that dtype on the CPU by tools/oracle/gen_golden.py) relative to the scale
    of the fp32 output: (mean err / mean|ref|, max err / max|ref|).  bf16: 1.8e-2 / 1.6e-2..., fp16: 2.3e-3 / ..."""
    if dtype not in _YARD:
        t = load_file(os.path.join(G, "unet_tiny.safetensors"))
        ref, low = t["motion/out"], t["motion/out_bf16" if dtype == torch.bfloat16 else "motion/out_fp16"]
        e = (low - ref).abs()
        _YARD[dtype] = (float(e.mean()) / float(ref.abs().mean()), float(e.max()) / float(ref.abs().max()))
    return _YARD[dtype]


def check(got, ref, dtype, lowp_ref=None):
    """f32 mode: north_star's rtol 1e-3 / atol 1e-4.  bf16 / fp16 mode: no worse than the reference's own forward in that
    dtype - against `lowp_ref` (the reference's low-precision output for the SAME inputs) when the goldens hold one: mean
    error <= 1.15x and max error <= 1.35x the reference's; otherwise against the relative yard-stick of the tiny motion UNet
    (mean <= 1.25x, max <= 2x, scaled by the tensor's own mean / max magnitude)."""
    got = got.float().cpu()
    if dtype == torch.float32:
        torch.testing.assert_close(got, ref, rtol=1e-3, atol=1e-4)
        return
    err = (got - ref).abs()
    if lowp_ref is not None:
        ref_err = (lowp_ref - ref).abs()
        assert float(err.mean()) <= 1.15 * float(ref_err.mean()), (float(err.mean()), float(ref_err.mean()))
        assert float(err.max()) <= 1.35 * float(ref_err.max()), (float(err.max()), float(ref_err.max()))
        return
    k_mean, k_max = yardstick(dtype)
    assert float(err.mean()) <= 1.25 * k_mean * float(ref.abs().mean()) + 1e-5, (float(err.mean()), float(ref.abs().mean()))
    assert float(err.max()) <= 2.0 * k_max * float(ref.abs().max()) + 1e-4, (float(err.max()), float(ref.abs().max()))


@pytest.fixture(scope="module")
def tiny():
    return load_file(os.path.join(G, "unet_tiny.safetensors"))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_unet_tiny_plain(tiny, dtype):
    x, ctx = cases.tiny_inputs(2, 4)
    m = build(cases.TINY, dtype)
    low = {torch.bfloat16: "plain/out_bf16", torch.float16: "plain/out_fp16"}.get(dtype)
    check(m(x[:, :, :2].to(DEV), 981, ctx.to(DEV)).sample, tiny["plain/out"], dtype, tiny[low] if low else None)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_unet_tiny_motion(tiny, dtype):
    x, ctx = cases.tiny_inputs(2, 4)
    m = build(cases.TINY_MOTION, dtype)
    low = {torch.bfloat16: "motion/out_bf16", torch.float16: "motion/out_fp16"}.get(dtype)
    check(m(x.to(DEV), torch.tensor(961), ctx.to(DEV)).sample, tiny["motion/out"], dtype, tiny[low] if low else None)


def test_unet_tiny_linear_projection(tiny):
    x, ctx = cases.tiny_inputs(2, 4)
    m = build(cases.TINY_LINEAR, torch.float32)
    check(m(x.to(DEV), 500, ctx.to(DEV), return_dict=False)[0], tiny["linear/out"], torch.float32)


def test_unet_tiny_controlnet_residuals(tiny):
    from tests.test_oracle_golden import ctrl_residuals
    x, ctx = cases.tiny_inputs(2, 4)
    down_res, mid_res = ctrl_residuals()
    m = build(cases.TINY_MOTION, torch.float32)
    y = m(x.to(DEV), 961, ctx.to(DEV), down_block_additional_residuals=tuple(r.to(DEV) for r in down_res),
          mid_block_additional_residual=mid_res.to(DEV)).sample
    check(y, tiny["motion/out_ctrl"], torch.float32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_reference_write_read(tiny, dtype):
    """ReferenceNet write -> fp16-rounded banks -> Backbone read with CFG batch 2."""
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.reference_control import ReferenceAttentionControl
    x, ctx = cases.tiny_inputs(2, 4)
    ref = build(cases.TINY, dtype, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    unet = build(cases.TINY_MOTION, dtype)
    writer = ReferenceAttentionControl(ref, do_classifier_free_guidance=True, mode="write", batch_size=1)
    reader = ReferenceAttentionControl(unet, do_classifier_free_guidance=True, mode="read", batch_size=1)
    ref_lat = seeded_randn((1, 4, 16, 16), 3).repeat(2, 1, 1, 1)
    ref(ref_lat.to(DEV), 961, encoder_hidden_states=ctx.to(DEV), return_dict=False)
    for i, p in enumerate(writer.order):
        check(writer.bank[p][0], tiny[f"banks/{i}"], dtype)
    reader.update(writer)
    y = unet(x.to(DEV), 961, ctx.to(DEV)).sample
    reader.clear()
    # low-precision gate = the reference's own read-path forward in that dtype (bf16: banks rounded through fp16 like update(),
    # then cast to the model dtype - the reference's literal fp16 banks do not run in a bf16 model, see gen_golden.run_reader)
    check(y, tiny["read/out"], dtype, {torch.float16: tiny["read/out_fp16"], torch.bfloat16: tiny["read/out_bf16"]}.get(dtype))
    if dtype == torch.float32:  # uc rows equal the no-bank run
        torch.testing.assert_close(y[:1].cpu(), tiny["motion/out"][:1], rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reference_write_read_fusion_blocks_full(tiny, dtype):
    """fusion_blocks="full" (mutual_self_attention.py:532-537): the down-path transformer blocks write / read banks too - all 16
    blocks, paired in the reference's order.  Goldens from the reference's own control object."""
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.reference_control import ReferenceAttentionControl
    x, ctx = cases.tiny_inputs(2, 4)
    ref = build(cases.TINY, dtype, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    unet = build(cases.TINY_MOTION, dtype)
    writer = ReferenceAttentionControl(ref, do_classifier_free_guidance=True, mode="write", batch_size=1, fusion_blocks="full")
    reader = ReferenceAttentionControl(unet, do_classifier_free_guidance=True, mode="read", batch_size=1, fusion_blocks="full")
    assert len(writer.order) == len(reader.order) == 16
    ref(seeded_randn((1, 4, 16, 16), 3).repeat(2, 1, 1, 1).to(DEV), 961, encoder_hidden_states=ctx.to(DEV), return_dict=False)
    for i, p in enumerate(writer.order):
        check(writer.bank[p][0], tiny[f"banks_full/{i}"], dtype)
    reader.update(writer)
    y = unet(x.to(DEV), 961, ctx.to(DEV)).sample
    reader.clear()
    check(y, tiny["read/out_full"], dtype)
    if dtype == torch.float32:
        assert float((y[1].cpu() - tiny["read/out"][1]).abs().max()) > 1e-2    # the down-path banks are live


@pytest.mark.parametrize("ref_group", [10, 2, 1])
@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("kind", ["ddim", "ddpm"])
def test_denoise_loop_vs_golden(kind, graphs, ref_group):
    """3 steps, 8 frames in overlapping windows of 4 - the loop of EMOAnimationPipeline.py:698-823.  ref_group = ReferenceNet
    timesteps per batched pass: 10 -> one group of 3; 2 -> groups [0,1],[2] (second HBM slot, look-ahead on the side stream);
    1 -> the reference's per-step order."""
    from emote_hack_amd import DDIMScheduler, DDPMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    g = load_file(os.path.join(G, "loop_tiny.safetensors"))
    ref = build(cases.TINY, torch.float32, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    unet = build(cases.TINY_MOTION, torch.float32)
    sch = DDIMScheduler() if kind == "ddim" else DDPMScheduler()
    pipe = EMOAnimationPipeline(unet=unet, scheduler=sch)
    lat, eps = pipe.denoise(seeded_randn((1, 4, 8, 16, 16), 5).to(DEV), seeded_randn((1, 4, 16, 16), 3), seeded_randn((2, 5, 32), 2),
                            appearance_encoder=ref, num_inference_steps=3, guidance_scale=7.5, context_frames=4,
                            context_stride=1, context_overlap=2, seed=0, return_eps=True, use_graphs=graphs,
                            reference_group=ref_group)
    for i in range(3):
        torch.testing.assert_close(eps[i].cpu(), g[f"{kind}/eps{i}"], rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(lat.cpu(), g[f"{kind}/latents"], rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("prefix,cbs,gs", [("ddim_cbs2", 2, 7.5), ("ddim_nocfg", 1, 1.0)])
def test_denoise_loop_context_batch_size_and_no_cfg_vs_golden(prefix, cbs, gs, graphs):
    """Goldens re-enacted around the reference's own UNet (tools/oracle/gen_golden.py gen_loop):
    ddim_cbs2 - context_batch_size 2 over three windows (a full batch + a partial one) with the reference's literal pairing at
        cbs > 1: `torch.cat([text] * cbs)` (:631) puts window 0's cond row under the UNCOND text and the bank written under it, so
        the ReferenceNet runs under both texts and the UNet calls are split per bank variant;
    ddim_nocfg - guidance_scale 1.0 (`do_classifier_free_guidance = guidance_scale > 1.0`, :622): cond units only, every row
        reads the bank, eps = noise_pred / counter (emo_sched_step with guidance_scale <= 1)."""
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    g = load_file(os.path.join(G, "loop_tiny.safetensors"))
    ref = build(cases.TINY, torch.float32, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    unet = build(cases.TINY_MOTION, torch.float32)
    pipe = EMOAnimationPipeline(unet=unet, scheduler=DDIMScheduler())
    text = seeded_randn((2, 5, 32), 2)
    lat, eps = pipe.denoise(seeded_randn((1, 4, 8, 16, 16), 5).to(DEV), seeded_randn((1, 4, 16, 16), 3), text if gs > 1 else text[1:],
                            appearance_encoder=ref, num_inference_steps=3, guidance_scale=gs, context_frames=4, context_stride=1,
                            context_overlap=2, seed=0, return_eps=True, use_graphs=graphs, context_batch_size=cbs)
    for i in range(3):
        torch.testing.assert_close(eps[i].cpu(), g[f"{prefix}/eps{i}"], rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(lat.cpu(), g[f"{prefix}/latents"], rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("graphs", [False, True])
def test_denoise_loop_multi_gpu_code_path_single_rank(graphs):
    """The multi-GPU branch of the loop (eps slices through the all_gather buffer, accumulate from the gathered rows) on ONE
    rank over RCCL: same goldens as the single-process loop.  (world_size > 1 is covered by the gloo tests on CPU; the driver
    runs the 8-GPU bench.)"""
    import socket
    import torch.distributed as td
    from emote_hack_amd import DDPMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    if td.is_initialized():
        pytest.skip("a process group already exists")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    td.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        g = load_file(os.path.join(G, "loop_tiny.safetensors"))
        ref = build(cases.TINY, torch.float32, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
        unet = build(cases.TINY_MOTION, torch.float32)
        pipe = EMOAnimationPipeline(unet=unet, scheduler=DDPMScheduler())
        lat, eps = pipe.denoise(seeded_randn((1, 4, 8, 16, 16), 5).to(DEV), seeded_randn((1, 4, 16, 16), 3), seeded_randn((2, 5, 32), 2),
                                appearance_encoder=ref, num_inference_steps=3, guidance_scale=7.5, context_frames=4,
                                context_stride=1, context_overlap=2, seed=0, return_eps=True, use_graphs=graphs,
                                dist=True, rank=0, world_size=1)
        torch.testing.assert_close(lat.cpu(), g["ddpm/latents"], rtol=1e-3, atol=1e-4)
    finally:
        td.destroy_process_group()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_shared_prefix_of_a_cfg_batch_is_the_same_forward(dtype):
    """The sampler's [uncond, cond] batch carries the same latents in both halves (EMOAnimationPipeline.py:759-763) and the two
    rows differ only from the first text cross-attention on: with _halves_identical the UNet runs conv_in, the first resnet and
    the first transformer's self-attention half ONCE on B / 2 rows and duplicates the result.  Same arithmetic - the outputs
    must agree with the plain forward (f32: to rounding of a different GEMM tile plan; bf16: to a bf16 ulp of the activations)."""
    x, ctx = cases.tiny_inputs(1, 4)
    x2 = x.repeat(2, 1, 1, 1, 1)
    ctx2 = torch.cat([ctx, seeded_randn(tuple(ctx.shape), 77)])
    m = build(cases.TINY_MOTION, dtype)
    y_plain = m(x2.to(DEV), 961, ctx2.to(DEV)).sample.float()
    y_dup = m(x2.to(DEV), 961, ctx2.to(DEV), _halves_identical=True).sample.float()
    assert float((y_plain[0] - y_plain[1]).abs().max()) > 1e-3          # the two rows do differ (different text)
    if dtype == torch.float32:
        torch.testing.assert_close(y_dup, y_plain, rtol=1e-4, atol=1e-5)
    else:       # two associations of the same arithmetic in bf16: inside the yard-stick every bf16 forward is held to
        _same_function(y_dup, y_plain, dtype)


def _same_function(y_a, y_b, dtype):
    """Two associations of the same arithmetic: f32 agrees to rounding; in bf16 the two differ by the rounding of an intermediate
    that one of them never stores - bounded by the bf16 yard-stick against the f32 goldens every forward is held to anyway
    (mean difference within 1.25x the reference's own bf16 mean error - the factor `check` uses for this yard-stick; behind the
    first differing rounding the two forwards are independent samples of the bf16 noise, their difference sits at ~1.0x: 1.0003x
    measured for the fused tail after the GEGLU product changed its association - and no element further than 1.5x its max error)."""
    if dtype == torch.float32:
        torch.testing.assert_close(y_a, y_b, rtol=1e-4, atol=2e-5)
        return
    mean_rel, max_rel = yardstick(dtype)
    d = (y_a - y_b).abs()
    assert float(d.mean()) <= 1.25 * mean_rel * float(y_b.abs().mean()), (float(d.mean()), mean_rel * float(y_b.abs().mean()))
    assert float(d.max()) <= 1.5 * max_rel * float(y_b.abs().max()), (float(d.max()), max_rel * float(y_b.abs().max()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_feed_forward_tail_is_the_same_forward(dtype):
    """FUSE_FF_TAIL: ff.net.2 (+ residual) and proj_out (+ residual) run as ONE GEMM over the side-by-side [g | h] buffer with
    the weights [Wo W2 | Wo] (attention.py:154-161,316-320; motion_module.py:215-227).  Same function, different association:
    f32 agrees to rounding, bf16 to the bf16 noise of one fewer rounding of the intermediate."""
    from emote_hack_amd import unet as unet_mod
    x, ctx = cases.tiny_inputs(2, 4)
    try:
        unet_mod.FUSE_FF_TAIL = False
        y_plain = build(cases.TINY_MOTION, dtype)(x.to(DEV), 961, ctx.to(DEV)).sample.float()
    finally:
        unet_mod.FUSE_FF_TAIL = True
    m = build(cases.TINY_MOTION, dtype)
    assert m._fuse_tail and any(k.endswith(".tail.w") for k in m._w)
    y_fused = m(x.to(DEV), 961, ctx.to(DEV)).sample.float()
    _same_function(y_fused, y_plain, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_groupnorm_folded_into_proj_in_is_the_same_forward(dtype):
    """GN_FOLD_MIN_HW: the per-frame GroupNorm of every transformer / motion module folded into per-frame proj_in weights
    (attention.py:124,135-146; motion_module.py:147-151).  The tiny model's frames (16x16) lie below the product threshold, so
    the threshold is lowered for this test; same function, the normalised tensor is just never rounded to the compute dtype."""
    from emote_hack_amd import unet as unet_mod
    x, ctx = cases.tiny_inputs(2, 4)
    m = build(cases.TINY_MOTION, dtype)
    keep = unet_mod.GN_FOLD_MIN_HW
    try:
        unet_mod.GN_FOLD_MIN_HW = 0
        y_plain = m(x.to(DEV), 961, ctx.to(DEV)).sample.float()
        unet_mod.GN_FOLD_MIN_HW = 256
        from emote_hack_amd import ops
        ops.PROFILER = ops.KernelProfiler()
        y_fold = m(x.to(DEV), 961, ctx.to(DEV)).sample.float()
        assert "groupnorm_fold" in ops.PROFILER.summary(), "the fold did not run"
    finally:
        unet_mod.GN_FOLD_MIN_HW = keep
        ops.PROFILER = None
    _same_function(y_fold, y_plain, dtype)


def test_pipeline_call_signature_and_errors():
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    ref = build(cases.TINY, torch.float32, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    unet = build(cases.TINY_MOTION, torch.float32)
    pipe = EMOAnimationPipeline(None, None, None, unet, None, DDIMScheduler())
    with pytest.raises(ValueError):
        pipe("", 4, height=130, width=128, appearance_encoder=ref)
    out = pipe("", 4, height=128, width=128, num_inference_steps=2, appearance_encoder=ref, context_frames=4,
               init_latents=seeded_randn((4, 4, 16, 16), 5), text_embeddings=seeded_randn((2, 5, 32), 2),
               ref_image_latents=seeded_randn((1, 4, 16, 16), 3), output_type="latent")
    assert tuple(out.videos.shape) == (1, 4, 4, 16, 16) and bool(torch.isfinite(out.videos).all())


def test_cfg1_baseline_config1():
    """BASELINE.json configs[0]: UNet from configs/unet-config.yaml:default, (1,4,1,32,32), t=981."""
    path = os.path.join(G, "cfg1.safetensors")
    cfg = dict(cases.SD15, norm_num_groups=4)
    m = build(cfg, torch.float32)
    y = m(seeded_randn((1, 4, 1, 32, 32), 1).to(DEV), 981, seeded_randn((1, 77, 768), 2).to(DEV)).sample
    check(y, load_file(path)["cfg1/out"], torch.float32)


def test_config4_geometry_fp16():
    """BASELINE.json configs[4] geometry: 768x768 (96x96 latents), a 24-frame window, speed-layer embeddings, fp16 - on a
    two-level SD-1.5-width UNet with motion modules.  fp16 HIP vs f32 HIP (the f32 path is pinned to the oracle at the
    small sizes above) within the fp16 yard-stick, and CFG batch rows independent of each other."""
    cfg = dict(cases.SD15_MOTION, block_out_channels=(320, 640), down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"),
               up_block_types=("UpBlock3D", "CrossAttnUpBlock3D"), attention_head_dim=8, layers_per_block=1)
    x, ctx = seeded_randn((2, 4, 24, 96, 96), 1), seeded_randn((2, 77, 768), 2)
    speed = 0.1 * seeded_randn((2, 4 * 320), 3)
    m32 = build(cfg, torch.float32)
    y32 = m32(x.to(DEV), 500, ctx.to(DEV), speed_embeddings=speed.to(DEV)).sample.float().cpu()
    del m32
    torch.cuda.empty_cache()
    m16 = build(cfg, torch.float16)
    y16 = m16(x.to(DEV), 500, ctx.to(DEV), speed_embeddings=speed.to(DEV)).sample
    assert y16.shape == (2, 4, 24, 96, 96) and bool(torch.isfinite(y16).all())
    check(y16, y32, torch.float16)
    y1 = m16(x[1:].to(DEV), 500, ctx[1:].to(DEV), speed_embeddings=speed[1:].to(DEV)).sample
    torch.testing.assert_close(y1.float().cpu(), y16[1:].float().cpu(), rtol=2e-2, atol=2e-2)


def test_cfg2_full_size_properties():
    """BASELINE.json configs[1] at FULL size (SD-1.5 widths + motion modules, 12 frames of 64x64 latents, CFG batch of 2):
    too large for the CPU oracle in a test, so size-independent properties - bf16 HIP vs f32 HIP (the f32 path is pinned to
    the oracle / reference goldens at the small sizes above) within the bf16 yard-stick, finite output, and the uncond /
    cond batch rows independent of each other."""
    x, ctx = seeded_randn((2, 4, 12, 64, 64), 1), seeded_randn((2, 77, 768), 2)
    m32 = build(cases.SD15_MOTION, torch.float32)
    y32 = m32(x.to(DEV), 981, ctx.to(DEV)).sample.float().cpu()
    y32_c = m32(x[1:].to(DEV), 981, ctx[1:].to(DEV)).sample.float().cpu()
    torch.testing.assert_close(y32_c, y32[1:], rtol=1e-3, atol=1e-4)
    del m32
    torch.cuda.empty_cache()
    m16 = build(cases.SD15_MOTION, torch.bfloat16)
    y16 = m16(x.to(DEV), 981, ctx.to(DEV)).sample
    assert bool(torch.isfinite(y16).all())
    check(y16, y32, torch.bfloat16)


def test_unet_vs_oracle_medium_size_properties():
    """A size the goldens do not hold (SD-1.5 widths at 16x16 latent, F=3, heads of 40/80/160): HIP f32
    vs the CPU oracle on the same seeded inputs; plus frame-permutation equivariance without motion
    modules is NOT expected (5-D GroupNorm couples frames) but batch rows must be independent."""
    from oracle import unet_ref as U
    from emote_hack_amd.spec import build_spec, param_shapes
    cfg = dict(cases.SD15_MOTION, block_out_channels=(320, 640), down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"),
               up_block_types=("UpBlock3D", "CrossAttnUpBlock3D"), attention_head_dim=8, layers_per_block=1)
    sd = synth_state_dict(param_shapes(build_spec(cfg)))
    x, ctx = seeded_randn((2, 4, 3, 16, 16), 1), seeded_randn((2, 9, 768), 2)
    ref = U.unet_forward(sd, cfg, x, 321, ctx)
    m = build(cfg, torch.float32)
    y = m(x.to(DEV), 321, ctx.to(DEV)).sample
    check(y, ref, torch.float32)
    y0 = m(x[:1].to(DEV), 321, ctx[:1].to(DEV)).sample
    torch.testing.assert_close(y0.cpu(), y[:1].cpu(), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("graphs", [False, True])
def test_motion_frame_conditioning_vs_oracle(graphs):
    """the previous clip's last frames go through the ReferenceNet next to the reference image and their LN1
    features join the reference banks as extra tokens (Lk1 = 3 * L here).  HIP f32 loop vs the oracle loop with the same
    motion latents; and the motion frames are live (the result differs from the run without them)."""
    from oracle.pipeline_ref import denoise_loop
    from oracle.scheduler_ref import SchedulerRef
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    from emote_hack_amd.spec import build_spec, param_shapes
    ref = build(cases.TINY, torch.float32, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    unet = build(cases.TINY_MOTION, torch.float32)
    usd = synth_state_dict(param_shapes(build_spec(cases.TINY_MOTION)))
    rsd = synth_state_dict(param_shapes(ref.spec), prefix=cases.REF_PREFIX)
    lat, refl, text = seeded_randn((1, 4, 4, 16, 16), 5), seeded_randn((1, 4, 16, 16), 3), seeded_randn((2, 5, 32), 2)
    motion = 0.5 * seeded_randn((2, 4, 16, 16), 6)
    kw = dict(num_inference_steps=2, guidance_scale=7.5, context_frames=4, context_stride=1, context_overlap=0, seed=0)
    want = denoise_loop(usd, cases.TINY_MOTION, rsd, cases.TINY, lat, refl, text, scheduler=SchedulerRef("ddim"), motion_latents=motion, **kw)
    base = denoise_loop(usd, cases.TINY_MOTION, rsd, cases.TINY, lat, refl, text, scheduler=SchedulerRef("ddim"), **kw)
    pipe = EMOAnimationPipeline(unet=unet, scheduler=DDIMScheduler())
    got = pipe.denoise(lat.to(DEV), refl, text, appearance_encoder=ref, use_graphs=graphs, motion_latents=motion, **kw)
    torch.testing.assert_close(got.cpu(), want, rtol=1e-3, atol=1e-4)
    assert float((want - base).abs().max()) > 1e-3
    if not graphs:   # clip chaining: the second clip sees the first one's tail, the first one zero maps
        clips = pipe.denoise_chained([lat.to(DEV), seeded_randn((1, 4, 4, 16, 16), 8).to(DEV)], refl, text, n_motion_frames=2,
                                     appearance_encoder=ref, **kw)
        z = denoise_loop(usd, cases.TINY_MOTION, rsd, cases.TINY, lat, refl, text, scheduler=SchedulerRef("ddim"),
                         motion_latents=torch.zeros(2, 4, 16, 16), **kw)
        torch.testing.assert_close(clips[0].cpu(), z, rtol=1e-3, atol=1e-4)
        nxt = denoise_loop(usd, cases.TINY_MOTION, rsd, cases.TINY, seeded_randn((1, 4, 4, 16, 16), 8), refl, text, scheduler=SchedulerRef("ddim"),
                           motion_latents=z[0, :, -2:].permute(1, 0, 2, 3), **kw)
        torch.testing.assert_close(clips[1].cpu(), nxt, rtol=2e-3, atol=2e-4)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_unet_non_multiple_of_8_input(tiny, dtype):
    """unet_controlnet.py:357-365,456-459: a 20x12 latent (not a multiple of 2^3) - stride-2 convs give 10x6, 5x3, 3x2 and the
    upsamplers interpolate (nearest) to the skip's size instead of x2 (emo_gemm_params.up_h / up_w).  Golden from the
    reference's own UNet."""
    m = build(cases.TINY_MOTION, dtype)
    y = m(seeded_randn((1, 4, 2, 20, 12), 1).to(DEV), 500, seeded_randn((1, 5, 32), 2).to(DEV)).sample
    check(y, tiny["motion/out_20x12"], dtype)


def test_denoise_loop_wrapped_window_with_repeated_frames():
    """uniform(20 frames, context 16, stride 2) emits a wrapped window that lists frames 0..10 twice
    (context.py:20-42).  The reference's `noise_pred[:, :, c] = noise_pred[:, :, c] + pred` is an index assignment: ONE
    occurrence per frame counts and the counter grows by one; WHICH occurrence is undefined in torch (a race in CUDA and in
    multi-threaded CPU index_put - this test was flaky while the oracle used the bare index assignment), so product and oracle
    pin the serial outcome: the last.  The accumulate kernel used to `+=` every occurrence non-atomically (a race); the host
    now marks the earlier duplicates.  HIP f32 loop vs the oracle loop."""
    from oracle.pipeline_ref import denoise_loop
    from oracle.scheduler_ref import SchedulerRef
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    from emote_hack_amd.spec import build_spec, param_shapes
    ref = build(cases.TINY, torch.float32, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    unet = build(cases.TINY_MOTION, torch.float32)
    usd = synth_state_dict(param_shapes(build_spec(cases.TINY_MOTION)))
    rsd = synth_state_dict(param_shapes(ref.spec), prefix=cases.REF_PREFIX)
    lat, refl, text = seeded_randn((1, 4, 20, 16, 16), 5), seeded_randn((1, 4, 16, 16), 3), seeded_randn((2, 5, 32), 2)
    kw = dict(num_inference_steps=2, guidance_scale=7.5, context_frames=16, context_stride=2, context_overlap=4, seed=0)
    want = denoise_loop(usd, cases.TINY_MOTION, rsd, cases.TINY, lat, refl, text, scheduler=SchedulerRef("ddim"), **kw)
    pipe = EMOAnimationPipeline(unet=unet, scheduler=DDIMScheduler())
    st = pipe.prepare_denoise(lat.to(DEV), refl, text, appearance_encoder=ref, **kw)
    assert any(int((fi < 0).sum()) > 0 for fi in st.frame_idx), "the wrapped window must carry dropped duplicates"
    got = pipe.denoise(lat.to(DEV), refl, text, appearance_encoder=ref, **kw)
    torch.testing.assert_close(got.cpu(), want, rtol=1e-3, atol=1e-4)


def test_call_entry_runs_the_graph_path_and_reuses_its_plan():
    """EMOAnimationPipeline.__call__ (EMOAnimationPipeline.py:544-578) must run what bench.py measures: HIP-graph replay by
    default, the prepared plan kept for the next clip.  (1) `pipe(...)` == `denoise(use_graphs=True)` bit for bit and both match
    the reference loop golden; (2) a second call with OTHER inputs of the same geometry re-arms the cached plan (same state
    object, graphs not re-captured) and equals a freshly prepared eager run bit for bit; (3) a different geometry re-plans."""
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    g = load_file(os.path.join(G, "loop_tiny.safetensors"))
    ref = build(cases.TINY, torch.float32, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    unet = build(cases.TINY_MOTION, torch.float32)
    pipe = EMOAnimationPipeline(unet=unet, scheduler=DDIMScheduler())
    lat, refl, text = seeded_randn((1, 4, 8, 16, 16), 5), seeded_randn((1, 4, 16, 16), 3), seeded_randn((2, 5, 32), 2)
    kw = dict(num_inference_steps=3, guidance_scale=7.5, context_frames=4, context_stride=1, context_overlap=2)
    call_kw = dict(video_length=8, height=128, width=128, output_type="latent", appearance_encoder=ref, seed=0, **kw)
    out = pipe("a prompt", latents=lat.to(DEV), text_embeddings=text, ref_image_latents=refl, **call_kw).videos
    st1 = pipe._plan_cache[1]
    assert st1.use_graphs and any(not isinstance(v, str) for v in st1.graphs.values()), "__call__ must capture and replay HIP graphs"
    want = pipe.denoise(lat.to(DEV), refl, text, appearance_encoder=ref, seed=0, use_graphs=True, **kw)
    assert torch.equal(out, want)
    torch.testing.assert_close(out.cpu(), g["ddim/latents"], rtol=1e-3, atol=1e-4)
    # (2) other inputs, same geometry: the plan and its graphs are reused
    lat2, refl2, text2 = seeded_randn((1, 4, 8, 16, 16), 15), seeded_randn((1, 4, 16, 16), 13), seeded_randn((2, 5, 32), 12)
    n_graphs = len(st1.graphs)
    out2 = pipe("a prompt", latents=lat2.to(DEV), text_embeddings=text2, ref_image_latents=refl2, **dict(call_kw, seed=3, guidance_scale=5.0))
    assert pipe._plan_cache[1] is st1 and len(st1.graphs) == n_graphs
    fresh = pipe.denoise(lat2.to(DEV), refl2, text2, appearance_encoder=ref, seed=3, use_graphs=False, **dict(kw, guidance_scale=5.0))
    assert torch.equal(out2.videos, fresh)
    assert not torch.equal(out2.videos, out)
    # and the first clip again through the re-armed plan
    out3 = pipe("a prompt", latents=lat.to(DEV), text_embeddings=text, ref_image_latents=refl, **call_kw).videos
    assert pipe._plan_cache[1] is st1 and torch.equal(out3, out)
    # (3) another geometry (4 frames = one window) prepares afresh
    out4 = pipe("a prompt", latents=lat[:, :, :4].to(DEV), text_embeddings=text, ref_image_latents=refl, **dict(call_kw, video_length=4)).videos
    assert pipe._plan_cache[1] is not st1
    want4 = pipe.denoise(lat[:, :, :4].to(DEV), refl, text, appearance_encoder=ref, seed=0, use_graphs=False, **kw)
    assert torch.equal(out4, want4)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["center", "class_table", "class_timestep", "class_identity"])
def test_unet_forward_switches_vs_reference(name, dtype):
    """center_input_sample (unet_controlnet.py:371-373) and the class embedding in its three ctor forms (:119-127,400-408) - off in every
    shipped config, run by the reference model for the goldens (tests/golden/unet_switches.safetensors)."""
    from tests.test_oracle_golden import SWITCH_CASES
    g = load_file(os.path.join(G, "unet_switches.safetensors"))
    extra, labels = SWITCH_CASES[name]
    m = build(dict(cases.TINY_MOTION, **extra), dtype)
    x, ctx = cases.tiny_inputs(2, 4)
    kw = dict(class_labels=labels().to(DEV)) if labels else {}
    check(m(x.to(DEV), 961, ctx.to(DEV), **kw).sample, g[name + "/out"], dtype)
    if labels:
        with pytest.raises(ValueError, match="class_labels"):
            m(x.to(DEV), 961, ctx.to(DEV))


def test_attention_mask_is_accepted_and_ignored_like_the_reference(tiny):
    """unet_controlnet.py:366-369 prepares the mask, no block of the reference uses it: same output with and without."""
    x, ctx = cases.tiny_inputs(2, 4)
    m = build(cases.TINY_MOTION, torch.float32)
    mask = (seeded_randn((2, 256), 72) > 0).float()
    y = m(x.to(DEV), 961, ctx.to(DEV), attention_mask=mask.to(DEV)).sample
    assert torch.equal(y, m(x.to(DEV), 961, ctx.to(DEV)).sample)
    g = load_file(os.path.join(G, "unet_switches.safetensors"))
    check(y, g["attention_mask/out"], torch.float32)


def test_invert_ddim_inversion_vs_the_reference_method():
    """EMOAnimationPipeline.invert (EMOAnimationPipeline.py:417-477) - DDIM inversion of four frames through the HIP UNet and the
    device branch of next_step (:379-400) - against the golden produced by the reference's own `invert` / `next_step` method bodies
    around the reference's UNet (tokenizer / text encoder / VAE stubbed by tensors): 5 steps scheduled, 3 taken."""
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    g = load_file(os.path.join(G, "pipeline_methods.safetensors"))
    pipe = EMOAnimationPipeline(unet=build(cases.TINY_MOTION, torch.float32), scheduler=DDIMScheduler())
    text, frames = seeded_randn((1, 5, 32), 503), seeded_randn((4, 4, 16, 16), 504)
    lat, inter = pipe.invert(None, "", num_inference_steps=5, num_actual_inference_steps=3, return_intermediates=True,
                             text_embeddings=text.to(DEV), latents=frames.to(DEV))
    assert len(inter) == 4
    torch.testing.assert_close(inter[1].float().cpu(), g["invert/step1"], rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(lat.float().cpu(), g["invert/latents"], rtol=1e-3, atol=1e-4)
    with pytest.raises(ValueError, match="text_embeddings"):
        pipe.invert(None, "", latents=frames.to(DEV))
    # the device branch of next_step against the host branch
    pipe.scheduler.set_timesteps(50)
    x, eps = seeded_randn((4, 4, 16, 16), 500), seeded_randn((4, 4, 16, 16), 501)
    xn, x0 = pipe.next_step(eps.to(DEV), 481, x.to(DEV))
    torch.testing.assert_close(xn.cpu(), g["next_step/481/x_next"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(x0.cpu(), g["next_step/481/pred_x0"], rtol=1e-5, atol=1e-5)
