"""GPU parity tests of the two UNet3DConditionModel ctor switches no shipped config turns on: unet_use_temporal_attention=True (the
attn_temp branch of BasicTransformerBlock, attention.py:235-246,309-318; mutual_self_attention.py:274-282) and
resnet_time_scale_shift="scale_shift" (resnet.py:149-156,191-195).  Model and module level against goldens captured from the reference's
own classes (tests/golden/unet_switches2.safetensors, tools/oracle/gen_golden_switches2.py); kernel level - the modulated GroupNorm entries
and the attn_temp branch at SD-1.5 block shapes - against fp32 torch written here.
f32: rtol 1e-3 / atol 1e-4; bf16 / fp16: tests.test_gpu_unet.check against the reference's own forward in that dtype."""
import os

import pytest
import torch
import torch.nn.functional as F
from safetensors.torch import load_file

from emote_hack_amd.synth import seeded_randn, synth_state_dict, synth_tensor
from tests import cases
from tests.test_gpu_kernels import DTYPES, TOL
from tests.test_gpu_unet import build, check

pytestmark = pytest.mark.gpu
DEV = "cuda"
TEMP = dict(unet_use_temporal_attention=True)
SS = dict(resnet_time_scale_shift="scale_shift")
MODELS = {"temp": (cases.TINY_MOTION, TEMP), "ss": (cases.TINY_MOTION, SS), "both": (cases.TINY_MOTION, dict(TEMP, **SS)),
          "both_linear": (cases.TINY_LINEAR, dict(TEMP, **SS))}
LOW = {torch.bfloat16: "_bf16", torch.float16: "_fp16"}
DTI = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


@pytest.fixture(scope="module")
def gold():
    return load_file(os.path.join(cases.GOLDEN_DIR, "unet_switches2.safetensors"))


def report(name, got, ref, low=None):
    """print the figures a bound is held against before it is asserted"""
    err = (got.float().cpu() - ref).abs()
    msg = f"[switches2] {name}: err mean {float(err.mean()):.3e} max {float(err.max()):.3e}; |ref| mean {float(ref.abs().mean()):.3e}"
    if low is not None:
        e2 = (low - ref).abs()
        msg += f"; reference's own low-precision err mean {float(e2.mean()):.3e} max {float(e2.max()):.3e}"
    print(msg)


# =============================================================================== model level
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(MODELS))
def test_switched_unet_vs_reference(gold, name, dtype):
    base, extra = MODELS[name]
    x, ctx = cases.tiny_inputs(2, 4)
    m = build(dict(base, **extra), dtype)
    if "temporal" in str(extra) and dtype == torch.float32:
        assert not any(k.endswith(".tail.w") and ".attentions." in k for k in m._w), "blocks with attn_temp take the unfused tail"
    y = m(x.to(DEV), 961, ctx.to(DEV)).sample
    low = gold[f"{name}/out{LOW[dtype]}"] if dtype in LOW else None
    report(f"{name}/out {dtype}", y, gold[f"{name}/out"], low)
    check(y, gold[f"{name}/out"], dtype, low)


@pytest.mark.parametrize("name", ["temp", "both"])
def test_layernorm_fold_off_is_the_same_forward(gold, name):
    """norm_temp through ops.layer_norm + GEMM instead of the folded q | k | v projection: the same goldens"""
    from emote_hack_amd import unet as unet_mod
    base, extra = MODELS[name]
    x, ctx = cases.tiny_inputs(2, 4)
    try:
        unet_mod.FOLD_LAYERNORM = False
        m = build(dict(base, **extra), torch.float32)
        assert not m._fold_ln and any(k.endswith(".norm_temp.g") for k in m._w)
        y = m(x.to(DEV), 961, ctx.to(DEV)).sample
    finally:
        unet_mod.FOLD_LAYERNORM = True
    check(y, gold[f"{name}/out"], torch.float32)


def test_groupnorm_inside_the_conv_carries_the_modulation(gold):
    """GN_CONV_MIN_HW > 0: norm2 -> modulate -> SiLU applied inside conv2 from the emo_groupnorm_coeffs_mod table - the same goldens"""
    from emote_hack_amd import ops, unet as unet_mod
    x, ctx = cases.tiny_inputs(2, 4)
    m = build(dict(cases.TINY_MOTION, **SS), torch.float32)
    keep, orig, modulated = unet_mod.GN_CONV_MIN_HW, ops.group_norm_coeffs, []

    def spy(*a, **k):
        modulated.append(k.get("mod") is not None)
        return orig(*a, **k)
    try:
        unet_mod.GN_CONV_MIN_HW = 64
        ops.group_norm_coeffs = spy
        y = m(x.to(DEV), 961, ctx.to(DEV)).sample
    finally:
        unet_mod.GN_CONV_MIN_HW = keep
        ops.group_norm_coeffs = orig
    assert any(modulated) and not all(modulated), "norm2's table carries the modulation, norm1's does not"
    check(y, gold["ss/out"], torch.float32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_write_read_with_attn_temp(gold, dtype):
    """ReferenceNet write -> fp16-rounded banks -> read with CFG batch 2 on the model with attn_temp: the branch runs at the same
    position of the bank-reading forward (mutual_self_attention.py:274-282).  Golden through the reference's own ReferenceAttentionControl."""
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.reference_control import ReferenceAttentionControl
    x, ctx = cases.tiny_inputs(2, 4)
    ref = build(cases.TINY, dtype, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    unet = build(dict(cases.TINY_MOTION, **TEMP), dtype)
    writer = ReferenceAttentionControl(ref, do_classifier_free_guidance=True, mode="write", batch_size=1)
    reader = ReferenceAttentionControl(unet, do_classifier_free_guidance=True, mode="read", batch_size=1)
    ref(seeded_randn((1, 4, 16, 16), 3).repeat(2, 1, 1, 1).to(DEV), 961, encoder_hidden_states=ctx.to(DEV), return_dict=False)
    reader.update(writer)
    y = unet(x.to(DEV), 961, ctx.to(DEV)).sample
    reader.clear()
    low = gold[f"temp/read_out{LOW[dtype]}"] if dtype in LOW else None
    report(f"temp/read_out {dtype}", y, gold["temp/read_out"], low)
    check(y, gold["temp/read_out"], dtype, low)
    if dtype == torch.float32:   # the uncond rows never see the bank: they equal the no-bank run
        torch.testing.assert_close(y[:1].cpu(), gold["temp/out"][:1], rtol=1e-3, atol=1e-4)
        assert float((y[1:].cpu() - gold["temp/out"][1:]).abs().max()) > 1e-2    # and the bank is live in the cond rows


def test_graph_replay_is_bit_identical_on_the_switched_model():
    """three steps of pipeline.denoise on the tiny model with both switches: HIP-graph replay == eager launches, bit for bit (the
    modulated GroupNorm and attn_temp make no host sync and no allocation outside the captured pool)"""
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    ref = build(cases.TINY, torch.float32, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    unet = build(dict(cases.TINY_MOTION, **TEMP, **SS), torch.float32)
    plain = build(cases.TINY_MOTION, torch.float32)
    out = {}
    for graphs in (False, True):
        pipe = EMOAnimationPipeline(unet=unet, scheduler=DDIMScheduler())
        out[graphs] = pipe.denoise(seeded_randn((1, 4, 8, 16, 16), 5).to(DEV), seeded_randn((1, 4, 16, 16), 3), seeded_randn((2, 5, 32), 2),
                                   appearance_encoder=ref, num_inference_steps=3, guidance_scale=7.5, context_frames=4, context_stride=1,
                                   context_overlap=2, seed=0, use_graphs=graphs)
    assert bool(torch.isfinite(out[True]).all())
    assert torch.equal(out[True], out[False])
    base = EMOAnimationPipeline(unet=plain, scheduler=DDIMScheduler()).denoise(
        seeded_randn((1, 4, 8, 16, 16), 5).to(DEV), seeded_randn((1, 4, 16, 16), 3), seeded_randn((2, 5, 32), 2), appearance_encoder=ref,
        num_inference_steps=3, guidance_scale=7.5, context_frames=4, context_stride=1, context_overlap=2, seed=0, use_graphs=True)
    assert float((out[True] - base).abs().max()) > 1e-2     # the switches are live in the loop


# =============================================================================== module level
def _with_module_weights(cfg, overrides):
    """the tiny UNet of `cfg` with the parameters under some prefixes replaced: overrides = {model prefix: golden module's seed salt}"""
    from emote_hack_amd.spec import build_spec, param_shapes
    from emote_hack_amd.unet import UNet3DConditionModel
    m = UNet3DConditionModel(**cfg)
    shapes = param_shapes(m.spec)
    sd = synth_state_dict(shapes)
    for prefix, salt in overrides.items():
        hit = [k for k in shapes if k.startswith(prefix + ".")]
        assert hit, prefix
        for k in hit:
            sd[k] = synth_tensor(salt + k[len(prefix) + 1:], shapes[k])
    return m, sd


@pytest.mark.parametrize("name,cin,cout,slot", [("resnet_ss_sc", 32, 64, "down_blocks.1.resnets.0"), ("resnet_ss_id", 64, 64, "down_blocks.1.resnets.1")])
def test_scale_shift_resnet_vs_reference_class(gold, name, cin, cout, slot):
    """ResnetBlock3D(time_embedding_norm="scale_shift") (resnet.py:113-207), with and without shortcut, F = 3: the HIP resnet of the tiny
    UNet's 32 -> 64 / 64 -> 64 slots carrying the golden module's weights"""
    from emote_hack_amd import ops
    from emote_hack_amd.unet import _Ctx
    m, sd = _with_module_weights(dict(cases.TINY, **SS), {slot: name + "."})
    m.load_state_dict(sd)
    m.to(DEV, torch.float32)
    r = next(r for b in m.spec.down for r in b.resnets if r.prefix == slot)
    assert (r.cin, r.cout, r.temb, r.scale_shift) == (cin, cout, 128, True)
    x, emb = seeded_randn((2, cin, 3, 8, 8), 211), seeded_randn((2, 128), 212)
    rows = ops.ncfhw_to_rows(x.to(DEV), torch.float32)
    temb_all = ops.gemm(ops.silu(emb.to(DEV)), m._w["temb_all.w"], m._w["temb_all.b"])
    y = m._resnet(r, rows, temb_all, _Ctx(2, 3, 8, 8), 8, 8)
    got = ops.rows_to_ncfhw(y, 2, cout, 3, 8, 8)
    report(name, got, gold[name + "/out"])
    check(got, gold[name + "/out"], torch.float32)


@pytest.mark.parametrize("fold", [True, False])
def test_transformer_block_with_attn_temp_vs_reference_class(gold, fold):
    """BasicTransformerBlock(unet_use_temporal_attention=True) at video_length 4 (attention.py:164-320): the HIP transformer of the tiny
    UNet's 64-channel, 4-head slot carrying the golden block's weights.  The Transformer3DModel shell around the block is taken out:
    norm + proj_in are stepped over, proj_out is the identity, so the slot returns block(x) + x."""
    from emote_hack_amd import ops, unet as unet_mod
    from emote_hack_amd.unet import _Ctx
    slot = "down_blocks.1.attentions.0"
    try:
        unet_mod.FOLD_LAYERNORM = fold
        m, sd = _with_module_weights(dict(cases.TINY, **TEMP), {slot + ".transformer_blocks.0": "btb_temp."})
        sd[slot + ".proj_out.weight"] = torch.eye(64).reshape(64, 64, 1, 1)
        sd[slot + ".proj_out.bias"] = torch.zeros(64)
        m.load_state_dict(sd)
        m.to(DEV, torch.float32)
    finally:
        unet_mod.FOLD_LAYERNORM = True
    assert m._fold_ln == fold
    a = next(a for b in m.spec.down for a in b.attentions if a is not None and a.prefix == slot)
    assert (a.channels, a.heads, a.ctx_dim, a.temporal) == (64, 4, 32, True)
    m._norm_proj_in = lambda x, p, nb, HW, groups: x
    x, ctx = seeded_randn((2 * 4, 16, 64), 213), seeded_randn((2 * 4, 5, 32), 214)
    rows = x.reshape(-1, 64).contiguous().to(DEV)
    y = m._transformer(a, rows, ctx.reshape(-1, 32).contiguous().to(DEV), 5, 1, _Ctx(2, 4, 4, 4), 4, 4)
    got = (y.cpu() - x.reshape(-1, 64)).reshape(8, 16, 64)
    report(f"btb_temp fold={fold}", got, gold["btb_temp/out"])
    torch.testing.assert_close(y.cpu().reshape(8, 16, 64), gold["btb_temp/out"] + x, rtol=1e-3, atol=1e-4)


# =============================================================================== kernel level: modulated GroupNorm
def _close_dev(got, ref, dtype, what=""):
    tol = TOL[dtype]
    err = (got.float() - ref).abs()
    print(f"[switches2] {what} {dtype}: err max {float(err.max()):.3e} mean {float(err.mean()):.3e}")
    torch.testing.assert_close(got.float(), ref, rtol=tol["rtol"], atol=tol["atol"])


def _gn_mod_case(N, S, C, G, dtype, seed):
    """inputs on the device (quantised to the compute dtype's grid) and the fp32 torch statement of resnet.py:191-197 on them"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randn(N * S, C, generator=g, device=DEV) * 2 + 0.5).to(dtype)
    gamma = 1 + 0.1 * torch.randn(C, generator=g, device=DEV)
    beta = 0.1 * torch.randn(C, generator=g, device=DEV)
    mod = torch.cat([0.5 * torch.randn(N, C, generator=g, device=DEV), torch.randn(N, C, generator=g, device=DEV)], 1).contiguous()   # |1 + s| stays O(1)
    return x, gamma, beta, mod


def _gn_mod_ref(x, gamma, beta, mod, N, S, C, G, eps, silu):
    s, t = torch.chunk(mod, 2, dim=1)
    h = F.group_norm(x.float().reshape(N, S, C).permute(0, 2, 1), G, gamma, beta, eps)
    h = h * (1 + s[:, :, None]) + t[:, :, None]
    return (F.silu(h) if silu else h).permute(0, 2, 1).reshape(N * S, C)


GN_SHAPES = [(2, 12 * 64 * 64, 320, 32, False), (2, 12 * 32 * 32, 640, 32, False), (2, 12 * 8 * 8, 1280, 32, True)]   # (N, S, C, G, one launch)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("N,S,C,G,one", GN_SHAPES)
def test_modulated_groupnorm_vs_torch(dtype, N, S, C, G, one, silu):
    """emo_groupnorm_stats + emo_groupnorm_apply_mod (the 64x64 and 32x32 levels' joint norms) and emo_groupnorm_mod (the 8x8 level's)
    through ops.group_norm(mod=), against fp32 torch: contiguous operands, then x / y / mod as column views of wider buffers."""
    from emote_hack_amd import _lib, ops
    assert _lib.load().emo_groupnorm_one_launch_ok(N, S, C, G, DTI[dtype]) == int(one)
    x, gamma, beta, mod = _gn_mod_case(N, S, C, G, dtype, 900 + C)
    ref = _gn_mod_ref(x, gamma, beta, mod, N, S, C, G, 1e-5, silu)
    ops.PROFILER = ops.KernelProfiler()
    try:
        got = ops.group_norm(x, gamma, beta, N, G, 1e-5, silu, mod=mod)
        tags = [tag for (_, tag) in ops.PROFILER.by_shape()]
    finally:
        ops.PROFILER = None
    assert tags == [f"M={N * S} C={C}{' silu' if silu else ''} mod{' 1L' if one else ''}"], tags
    _close_dev(got, ref, dtype, f"gn_mod N={N} S={S} C={C} silu={silu}")
    plain = ops.group_norm(x, gamma, beta, N, G, 1e-5, silu)
    assert float((plain.float() - ref).abs().max()) > 0.1       # the modulation is live
    # strided: x with ldx > C, y with ldy > C (untouched around), mod a column view of a wider f32 buffer (the batched temb GEMM's output)
    xw = torch.zeros(N * S, C + 64, device=DEV, dtype=dtype)
    xw[:, 32:32 + C] = x
    yw = torch.zeros(N * S, C + 32, device=DEV, dtype=dtype)
    modw = torch.full((N, 2 * C + 24), 7.0, device=DEV)
    modw[:, 8:8 + 2 * C] = mod
    ops.group_norm(xw[:, 32:32 + C], gamma, beta, N, G, 1e-5, silu, out=yw[:, 16:16 + C], mod=modw[:, 8:8 + 2 * C])
    assert torch.equal(yw[:, 16:16 + C], got) and not yw[:, :16].any() and not yw[:, 16 + C:].any()
    # in place, as norm2 of the resnet runs it
    xi = x.clone()
    ops.group_norm(xi, gamma, beta, N, G, 1e-5, silu, out=xi, mod=mod)
    assert torch.equal(xi, got)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,S,C,G", [s[:4] for s in GN_SHAPES] + [(3, 1000, 2560, 32), (2, 100, 1536, 3)])
def test_modulated_groupnorm_coefficients(dtype, N, S, C, G):
    """emo_groupnorm_coeffs_mod: (i) the table against the fp32 statement scale' = rstd gamma (1 + s), shift' = (beta - mean rstd gamma)
    (1 + s) + t; (ii) BIT-identical to the factors emo_groupnorm_apply_mod uses.  The apply kernel computes y = x a + b from the SAME
    partials whatever rows it is handed, so its factors can be read back exactly: rows of zeros give y = b; rows of 2^40 give
    y = 2^80 a (b, O(1), lies below half an ulp of 2^80 a unless |a| < 2^-56 |b|, and scaling by a power of two is exact).  f32 reads
    both back exactly; bf16 reads them rounded to bf16 (2^80 is representable); fp16 cannot hold 2^80 and checks b alone.
    (C = 2560 runs the column-part split of the kernels; C = 1536 in 3 groups cannot split and runs their wide-row path in f32.)"""
    from emote_hack_amd import _lib, ops
    lib = _lib.load()
    x, gamma, beta, mod = _gn_mod_case(N, S, C, G, dtype, 950 + C)
    modw = torch.zeros(N, 2 * C + 8, device=DEV)
    modw[:, 4:4 + 2 * C] = mod
    mv = modw[:, 4:4 + 2 * C]
    coef = ops.group_norm_coeffs(x, gamma, beta, N, G, 1e-5, mod=mv)
    assert tuple(coef.shape) == (N, 2 * C)
    cf = coef.reshape(N, C // 2, 2, 2)                  # channel pairs interleaved (scale, scale, shift, shift)
    a, b = cf[:, :, 0, :].reshape(N, C), cf[:, :, 1, :].reshape(N, C)
    # (i) against torch, in f64 from the same rows
    xg = x.double().reshape(N, S, G, C // G)
    mean_c = xg.mean((1, 3)).repeat_interleave(C // G, 1)
    rstd_c = (xg.var((1, 3), unbiased=False) + 1e-5).rsqrt().repeat_interleave(C // G, 1)
    s, t = torch.chunk(mod.double(), 2, dim=1)
    a_ref = rstd_c * gamma.double() * (1 + s)
    b_ref = (beta.double() - mean_c * rstd_c * gamma.double()) * (1 + s) + t
    torch.testing.assert_close(a.double(), a_ref, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(b.double(), b_ref, rtol=1e-4, atol=1e-4)
    # the unmodulated table differs
    assert not torch.equal(ops.group_norm_coeffs(x, gamma, beta, N, G, 1e-5), coef)
    # (ii) the apply kernel's own factors, read back through it
    st = torch.cuda.current_stream().cuda_stream
    part = torch.empty(lib.emo_groupnorm_workspace_bytes(N, S, C, G) // 4, device=DEV, dtype=torch.float32)
    coef2 = torch.empty_like(coef)
    assert lib.emo_groupnorm_stats(x.data_ptr(), C, part.data_ptr(), N, S, C, G, DTI[dtype], st) == 0
    assert lib.emo_groupnorm_coeffs_mod(part.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mv.data_ptr(), mv.stride(0), coef2.data_ptr(), N, S, C, G,
                                        1e-5, DTI[dtype], st) == 0
    assert torch.equal(coef2, coef)
    y = torch.empty_like(x)

    def apply_to(rows):
        assert lib.emo_groupnorm_apply_mod(rows.data_ptr(), C, part.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mv.data_ptr(), mv.stride(0),
                                           y.data_ptr(), C, N, S, C, G, 1e-5, 0, DTI[dtype], st) == 0
        return y.reshape(N, S, C).clone()
    y0 = apply_to(torch.zeros_like(x))
    assert torch.equal(y0, b.to(dtype)[:, None, :].expand(N, S, C))
    if dtype != torch.float16:
        big = 2.0 ** 80
        ya = apply_to(torch.full_like(x, big))
        assert torch.equal(ya.float() / big, a.to(dtype).float()[:, None, :].expand(N, S, C))


def test_modulated_groupnorm_refusals_launch_nothing():
    from emote_hack_amd import _lib
    lib = _lib.load()
    N, S, C, G = 8, 64, 64, 8
    assert lib.emo_groupnorm_one_launch_ok(N, S, C, G, 0) == 1
    x = torch.zeros(N * S, C, device=DEV)
    y = torch.full_like(x, 3.0)
    gamma, beta, mod = torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(N, 2 * C + 4, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda m, ld: lib.emo_groupnorm_mod(x.data_ptr(), C, gamma.data_ptr(), beta.data_ptr(), m, ld, y.data_ptr(), C, N, S, C, G, 1e-5, 0, 0, st)
    assert call(None, 2 * C) != 0                                   # null mod
    assert call(mod.data_ptr(), 2 * C - 4) != 0                     # rows narrower than (scale | shift)
    assert call(mod.data_ptr() + 4, 2 * C + 4) != 0                 # not 16-byte aligned
    assert call(mod.data_ptr(), 2 * C + 2) != 0                     # a row stride that breaks the alignment of the next row
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())
    assert call(mod.data_ptr(), 2 * C + 4) == 0


# =============================================================================== kernel level: attn_temp at SD-1.5 block shapes
def _attn_temp_ref(h, gamma, beta, wq, wk, wv, wo, bo, B, Fr, HW, heads):
    """fp32 torch statement of attention.py:309-318: (b f) d c -> (b d) f c, norm_temp, q / k / v, softmax over the F frames, to_out,
    + residual, regrouped back"""
    C = h.shape[1]
    d = C // heads
    t = h.float().reshape(B, Fr, HW, C).permute(0, 2, 1, 3).reshape(B * HW, Fr, C)
    n = F.layer_norm(t, (C,), gamma, beta, 1e-5)
    q, k, v = (F.linear(n, w_).reshape(B * HW, Fr, heads, d).transpose(1, 2) for w_ in (wq, wk, wv))
    p = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, -1)
    o = (p @ v).transpose(1, 2).reshape(B * HW, Fr, C)
    o = F.linear(o, wo, bo) + t
    return o.reshape(B, HW, Fr, C).permute(0, 2, 1, 3).reshape(B * Fr * HW, C)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("B,Fr,HW,C,heads", [(2, 12, 64 * 64, 320, 8), (2, 12, 8 * 8, 1280, 8), (2, 12, 16 * 16, 640, 10), (2, 4, 16 * 16, 32, 4),
                                             (2, 4, 4 * 4, 64, 4)])
def test_attn_temp_branch_vs_torch(dtype, fold, B, Fr, HW, C, heads):
    """UNet._attn_temp - norm_temp (folded into the GEMM, or ops.layer_norm) -> q | k | v GEMM -> emo_temporal_attention -> to_out +
    residual - at the SD-1.5 block shapes (d = 40 at 64x64, d = 160 at 8x8), the `v2` section's head dim 64, and the tiny configs'
    d = 8 / 16 at F = 4: no shape these blocks produce is refused by the temporal kernel."""
    from emote_hack_amd.unet import UNet3DConditionModel, ln_fold_weights
    g = torch.Generator(device=DEV).manual_seed(1000 + C + HW)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    h = rn(B * Fr * HW, C).to(dtype)
    gamma, beta = 1 + 0.1 * rn(C), 0.1 * rn(C)
    wq, wk, wv, wo = (rn(C, C) / C ** 0.5 for _ in range(4))
    bo = 0.1 * rn(C)
    tb = "tb"
    m = UNet3DConditionModel.__new__(UNet3DConditionModel)      # the branch alone: its packed operands, no model around it
    m._fold_ln = fold
    wqkv = torch.cat([wq, wk, wv], 0)
    m._w = {tb + ".attn_temp.o.w": wo.to(dtype).contiguous(), tb + ".attn_temp.o.b": bo}
    if fold:
        m._w[tb + ".attn_temp.qkv_ln"] = ln_fold_weights(wqkv, None, gamma, beta, dtype)
    else:
        m._w.update({tb + ".attn_temp.qkv": wqkv.to(dtype).contiguous(), tb + ".norm_temp.g": gamma, tb + ".norm_temp.b": beta})
    got = m._attn_temp(tb, h, B, Fr, HW, heads, C // heads)
    q_ = lambda w_: w_.to(dtype).float()                         # the weights the kernels multiply by
    ref = _attn_temp_ref(h, gamma, beta, q_(wq), q_(wk), q_(wv), q_(wo), bo, B, Fr, HW, heads)
    _close_dev(got, ref, dtype, f"attn_temp B={B} F={Fr} HW={HW} C={C} heads={heads} fold={fold}")
    assert float((got.float() - h.float()).abs().max()) > 0.1    # the branch is live
