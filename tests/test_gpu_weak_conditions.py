"""The two weak conditions of the Backbone on the GPU: a face-region map behind conv_in and a head-speed embedding per frame.
Kernel level (emo_add_periodic, emo_mask_pool, the per-frame GroupNorm modulation), the UNet against the CPU restatement of
tests/weak_conditions_ref.py, same-function checks, the prepared / graph-captured sampling loop and `__call__`.

Tolerances: TOL of tests/test_gpu_kernels.py for the GroupNorm kernels - the table tests/norm_sweep_cases.py's sweeps hold the instance
form to (imported, with the sweeps' dtype list) -, `check` / `_same_function` of tests/test_gpu_unet.py at model level."""
import pytest
import torch
import torch.nn.functional as F

from emote_hack_amd.synth import seeded_randn, synth_state_dict
from tests import cases
from tests import norm_sweep_cases as NS
from tests import weak_conditions_ref as R
from tests.test_gpu_kernels import DEV, TOL
from tests.test_gpu_unet import _same_function, build, check

pytestmark = pytest.mark.gpu
DTYPES = NS.DTYPES
DTI = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def _ops():
    from emote_hack_amd import ops
    return ops


def _hip_error():
    from emote_hack_amd._lib import EmoHipError
    return EmoHipError


def _dev_randn(shape, seed, dtype=torch.float32):
    return seeded_randn(shape, seed).to(DEV).to(dtype)


# =============================================================================== emo_add_periodic
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 40])
def test_add_periodic(dtype, C):
    """y[m] = x[m] + f[m % P] on column views of wider buffers (ld > C), into a second buffer and IN PLACE: the f32 sum rounded once is
    exactly (x.float() + f.float()[m % P]).to(dtype)."""
    ops = _ops()
    P, M = 7, 28
    xw, fw = _dev_randn((M, C + 16), 100 + C, dtype), _dev_randn((P, C + 8), 200 + C, dtype)
    x, f = xw[:, 8:8 + C], fw[:, :C]
    want = (x.float() + f.float()[torch.arange(M, device=DEV) % P]).to(dtype)
    yw = torch.zeros(M, C + 24, device=DEV, dtype=dtype)
    got = ops.add_periodic(x, f, out=yw[:, 16:16 + C])
    assert got.data_ptr() == yw[:, 16:16 + C].data_ptr()
    assert torch.equal(yw[:, 16:16 + C], want) and not yw[:, :16].any() and not yw[:, 16 + C:].any()
    keep = xw.clone()
    assert ops.add_periodic(x, f).data_ptr() == x.data_ptr()                       # in place: the caller's slot keeps its address
    assert torch.equal(x, want) and torch.equal(xw[:, :8], keep[:, :8]) and torch.equal(xw[:, 8 + C:], keep[:, 8 + C:])


def test_add_periodic_refuses_a_partial_period():
    ops = _ops()
    x, f = torch.full((27, 8), 3.0, device=DEV), torch.ones(7, 8, device=DEV)
    with pytest.raises(_hip_error(), match="whole number of periods"):
        ops.add_periodic(x, f)
    torch.cuda.synchronize()
    assert bool((x == 3.0).all())


# =============================================================================== emo_mask_pool
@pytest.mark.parametrize("dtype", DTYPES)
def test_mask_pool(dtype):
    """16 x 24 -> 2 x 3 cells: channel 0 the 8 x 8 area mean, channels 1..7 zero.  A 0 / 1 mask and thresholded logits give k / 64,
    exact in every dtype (bf16 holds 8 significant bits); a float mask in f32 agrees with avg_pool2d to the summation-order bound
    64 * 2^-24 for |x| <= 1."""
    ops = _ops()
    g = torch.Generator().manual_seed(7)
    mask = (torch.rand(16, 24, generator=g) < 0.4)
    mask[:8, :8] = True                                              # a full cell (64 / 64) and an empty one
    mask[8:, 16:] = False
    got = ops.mask_pool(mask.float().to(DEV).contiguous(), dtype)
    assert tuple(got.shape) == (6, 8) and got.dtype == dtype
    assert torch.equal(got[:, 0].cpu(), R.pooled_mask(mask).reshape(6).to(dtype)) and not got[:, 1:].any()
    assert float(got[0, 0]) == 1.0 and float(got[5, 0]) == 0.0
    logits = seeded_randn((16, 24), 8)
    logits[3, 5] = 0.0                                               # x > 0 is strict: a zero logit is outside
    got = ops.mask_pool(logits.to(DEV).contiguous(), dtype, threshold=0.0)
    assert torch.equal(got[:, 0].cpu(), R.pooled_mask(logits, 0.0).reshape(6).to(dtype)) and not got[:, 1:].any()
    if dtype == torch.float32:
        soft = torch.rand(16, 24, generator=g)
        got = ops.mask_pool(soft.to(DEV).contiguous(), dtype)
        torch.testing.assert_close(got[:, 0].cpu(), F.avg_pool2d(soft[None, None], 8).reshape(6), rtol=0.0, atol=64 * 2.0 ** -24)
        assert not got[:, 1:].any()


def test_mask_pool_refuses_sizes_that_are_no_multiple_of_8():
    ops = _ops()
    for hw in ((12, 24), (16, 20)):
        with pytest.raises(_hip_error(), match="multiples of 8"):
            ops.mask_pool(torch.zeros(*hw, device=DEV), torch.float32)


# =============================================================================== per-frame GroupNorm modulation
def _gn_case(N, Fr, HW, C, G, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randn(N * Fr * HW, C, generator=g, device=DEV) * 2 + 0.5).to(dtype)
    gamma = 1 + 0.1 * torch.randn(C, generator=g, device=DEV)
    beta = 0.1 * torch.randn(C, generator=g, device=DEV)
    modw = torch.full((N * Fr, 2 * C + 8), 7.0, device=DEV)          # mod is a column view of a wider f32 buffer, as in the UNet
    modw[:, 4:4 + C] = 0.5 * torch.randn(N * Fr, C, generator=g, device=DEV)
    modw[:, 4 + C:4 + 2 * C] = torch.randn(N * Fr, C, generator=g, device=DEV)
    return x, gamma, beta, modw[:, 4:4 + 2 * C]


def _gn_ref(x, gamma, beta, mod, N, Fr, HW, C, G, eps, silu):
    """f32 torch: statistics joint over the F frames of an instance, (scale | shift) per frame"""
    h = F.group_norm(x.float().reshape(N, Fr * HW, C).permute(0, 2, 1), G, gamma, beta, eps).reshape(N, C, Fr, HW)
    s, t = torch.chunk(mod.reshape(N, Fr, 2 * C), 2, dim=2)
    h = h * (1 + s.permute(0, 2, 1)[..., None]) + t.permute(0, 2, 1)[..., None]
    return (F.silu(h) if silu else h).reshape(N, C, Fr * HW).permute(0, 2, 1).reshape(N * Fr * HW, C)


# (N, F, HW, C, G): the two small shapes run the two-launch pair (N = 2 gives the one-launch kernel too few blocks); the others - so that
# every kernel with a per-frame form runs - the one-launch kernel, the column-part split (C = 2560) and the wide-row arm (C = 1536 in f32)
GN_SHAPES = [(2, 3, 5, 16, 4), (2, 3, 5, 24, 3), (8, 2, 32, 64, 8), (2, 2, 210, 2560, 32), (2, 2, 50, 1536, 3)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("N,Fr,HW,C,G", GN_SHAPES)
def test_groupnorm_per_frame_modulation(dtype, silu, N, Fr, HW, C, G):
    from emote_hack_amd import _lib
    ops = _ops()
    one = bool(_lib.load().emo_groupnorm_one_launch_ok(N, Fr * HW, C, G, DTI[dtype]))
    assert one == ((N, C) == (8, 64))
    x, gamma, beta, mod = _gn_case(N, Fr, HW, C, G, dtype, 1000 + C)
    ref = _gn_ref(x, gamma, beta, mod, N, Fr, HW, C, G, 1e-5, silu)
    xw = torch.zeros(N * Fr * HW, C + 16, device=DEV, dtype=dtype)    # x with ldx > C, y in place (as norm2 of the resnet runs it)
    xw[:, 8:8 + C] = x
    got = ops.group_norm(xw[:, 8:8 + C], gamma, beta, N, G, 1e-5, silu, out=xw[:, 8:8 + C], mod=mod, mod_rows=HW)
    err = (got.float() - ref).abs()
    print(f"[weak] gn per-frame N={N} F={Fr} HW={HW} C={C} G={G} silu={silu} {dtype}: err max {float(err.max()):.3e} mean {float(err.mean()):.3e}")
    torch.testing.assert_close(got.float(), ref, **TOL[dtype])
    assert not xw[:, :8].any() and not xw[:, 8 + C:].any()
    # the frames are live: the instance form with frame 0's row differs
    inst = ops.group_norm(x, gamma, beta, N, G, 1e-5, silu, mod=mod[::Fr])
    assert float((inst.float() - ref).abs().max()) > 0.1
    # ... and with ONE row shared by all frames of an instance the per-frame entry is the instance entry, bit for bit
    shared = mod[::Fr].repeat_interleave(Fr, 0).contiguous()
    assert torch.equal(ops.group_norm(x, gamma, beta, N, G, 1e-5, silu, mod=shared, mod_rows=HW), inst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,Fr,HW,C,G", GN_SHAPES)
def test_groupnorm_per_frame_coefficients(dtype, N, Fr, HW, C, G):
    """emo_groupnorm_coeffs_mod_rows: one table row per frame, a' = rstd gamma (1 + s_f), b' = (beta - mean rstd gamma)(1 + s_f) + t_f with
    the instance's statistics (f64 statement, the bounds the instance table is held to); rows of one shared mod row are the instance table's."""
    ops = _ops()
    x, gamma, beta, mod = _gn_case(N, Fr, HW, C, G, dtype, 1100 + C)
    coef = ops.group_norm_coeffs(x, gamma, beta, N, G, 1e-5, mod=mod, mod_rows=HW)
    assert tuple(coef.shape) == (N * Fr, 2 * C)
    cf = coef.reshape(N * Fr, C // 2, 2, 2)
    a, b = cf[:, :, 0, :].reshape(N * Fr, C), cf[:, :, 1, :].reshape(N * Fr, C)
    xg = x.double().reshape(N, Fr * HW, G, C // G)
    mean_c = xg.mean((1, 3)).repeat_interleave(C // G, 1).repeat_interleave(Fr, 0)
    rstd_c = (xg.var((1, 3), unbiased=False) + 1e-5).rsqrt().repeat_interleave(C // G, 1).repeat_interleave(Fr, 0)
    s, t = torch.chunk(mod.double(), 2, dim=1)
    torch.testing.assert_close(a.double(), rstd_c * gamma.double() * (1 + s), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(b.double(), (beta.double() - mean_c * rstd_c * gamma.double()) * (1 + s) + t, rtol=1e-4, atol=1e-4)
    inst = ops.group_norm_coeffs(x, gamma, beta, N, G, 1e-5, mod=mod[::Fr])
    shared = mod[::Fr].repeat_interleave(Fr, 0).contiguous()
    assert torch.equal(ops.group_norm_coeffs(x, gamma, beta, N, G, 1e-5, mod=shared, mod_rows=HW), inst.repeat_interleave(Fr, 0))


# =============================================================================== the UNet against the restatement
SPEED_SEED, MASK_SEED = 41, 42


def _controller(dtype, cout=32):
    from emote_hack_amd.conditioning import FaceRegionController
    ctl = FaceRegionController(1, cout)
    sd = synth_state_dict(ctl.state_dict_shapes(), prefix="face_region.")
    ctl.load_state_dict(sd)
    return ctl.to(DEV, dtype), sd


def _latent_mask(h=16, w=16):
    m = (seeded_randn((h, w), MASK_SEED) > 0).float()
    m[4:9, 3:12] = 1.0
    return m


def _face_rows(ctl, mask, dtype):
    rows = _ops().ncfhw_to_rows(mask.reshape(1, 1, 1, *mask.shape).to(DEV), dtype, cpad=8)
    return ctl.forward_rows(rows, 1, *mask.shape)


VARIANTS = {"default": cases.TINY_MOTION, "scale_shift": dict(cases.TINY_MOTION, **R.SS)}
CASES = ("speed", "face", "both")


@pytest.fixture(scope="module")
def want():
    """the CPU restatement, once per (variant, case), on tiny_inputs() (B = 2, F = 4, 16 x 16)"""
    from emote_hack_amd.spec import build_spec, param_shapes
    x, ctx = cases.tiny_inputs(2, 4)
    speed = 0.5 * seeded_randn((2, 4, 128), SPEED_SEED)
    face = R.face_map(_controller(torch.float32)[1], _latent_mask()[None, None])
    out = {"x": x, "ctx": ctx, "speed": speed, "face": face}
    for name, cfg in VARIANTS.items():
        sd = synth_state_dict(param_shapes(build_spec(cfg)))
        out[name, "none"] = R.unet_forward(sd, cfg, x, 961, ctx)
        for case in CASES:
            out[name, case] = R.unet_forward(sd, cfg, x, 961, ctx, speed=speed if case != "face" else None, face=face if case != "speed" else None)
            assert float((out[name, case] - out[name, "none"]).abs().max()) > 1e-2, "the condition must be live in the restatement"
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_unet_weak_conditions_vs_restatement(want, variant, case, dtype):
    m = build(VARIANTS[variant], dtype)
    kw = {}
    if case != "face":
        kw["speed_embeddings"] = want["speed"].to(DEV)
    if case != "speed":
        kw["face_features"] = _face_rows(_controller(dtype)[0], _latent_mask(), dtype)
    y = m(want["x"].to(DEV), 961, want["ctx"].to(DEV), **kw).sample
    ref = want[variant, case]
    err = (y.float().cpu() - ref).abs()
    print(f"[weak] unet {variant} {case} {dtype}: err max {float(err.max()):.3e} mean {float(err.mean()):.3e}; |ref| mean {float(ref.abs().mean()):.3e}")
    check(y, ref, dtype)


def test_unet_face_features_as_a_map_and_argument_errors(want):
    m = build(cases.TINY_MOTION, torch.float32)
    ctl = _controller(torch.float32)[0]
    x, ctx = want["x"].to(DEV), want["ctx"].to(DEV)
    y_rows = m(x, 961, ctx, face_features=_face_rows(ctl, _latent_mask(), torch.float32)).sample
    fmap = ctl(_latent_mask()[None, None].to(DEV))                       # (1, C0, h, w) f32 through the NCHW entry
    torch.testing.assert_close(fmap.cpu(), want["face"], rtol=1e-3, atol=1e-4)
    _same_function(m(x, 961, ctx, face_features=fmap).sample.float(), y_rows.float(), torch.float32)
    for bad in (torch.zeros(255, 32, device=DEV), torch.zeros(256, 16, device=DEV), torch.zeros(2, 32, 16, 16), torch.zeros(256, 32, device=DEV).half()):
        with pytest.raises(ValueError, match="face_features"):
            m(x, 961, ctx, face_features=bad)
    for bad in (torch.zeros(2, 3, 128), torch.zeros(2, 4, 64), torch.zeros(1, 4, 128)):
        with pytest.raises(ValueError, match="per-frame speed_embeddings"):
            m(x, 961, ctx, speed_embeddings=bad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_equal_per_frame_speeds_are_the_per_clip_form(variant, dtype):
    x, ctx = cases.tiny_inputs(2, 4)
    sp = 0.5 * seeded_randn((2, 128), SPEED_SEED)
    m = build(VARIANTS[variant], dtype)
    y2 = m(x.to(DEV), 961, ctx.to(DEV), speed_embeddings=sp.to(DEV)).sample.float()
    y3 = m(x.to(DEV), 961, ctx.to(DEV), speed_embeddings=sp[:, None].expand(2, 4, 128).contiguous().to(DEV)).sample.float()
    assert float((y2 - m(x.to(DEV), 961, ctx.to(DEV)).sample.float()).abs().max()) > 1e-2
    _same_function(y3, y2, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_per_frame_speeds_with_the_groupnorm_inside_the_conv(variant, dtype):
    """GN_CONV_MIN_HW: where the halo conv normalises its own input (the 16 x 16 level here) conv1 takes the per-frame row bias next to
    the GroupNorm fold and a scale-shift conv2 reads a coefficient table with one row per FRAME (emo_groupnorm_coeffs_mod_rows, one
    image per table row): the same forward as the GroupNorm kernels in front of the conv."""
    from emote_hack_amd import unet as unet_mod
    ops = _ops()
    x, ctx = cases.tiny_inputs(2, 4)
    sp = (0.5 * seeded_randn((2, 4, 128), SPEED_SEED)).to(DEV)
    m = build(VARIANTS[variant], dtype)
    keep = unet_mod.GN_CONV_MIN_HW
    try:
        unet_mod.GN_CONV_MIN_HW = 0
        y_plain = m(x.to(DEV), 961, ctx.to(DEV), speed_embeddings=sp).sample.float()
        unet_mod.GN_CONV_MIN_HW = 256
        ops.PROFILER = ops.KernelProfiler()
        y_fold = m(x.to(DEV), 961, ctx.to(DEV), speed_embeddings=sp).sample.float()
        assert "groupnorm_stats" in ops.PROFILER.summary(), "the fold did not run"
    finally:
        unet_mod.GN_CONV_MIN_HW = keep
        ops.PROFILER = None
    _same_function(y_fold, y_plain, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_zero_face_features_are_no_face_features(dtype):
    x, ctx = cases.tiny_inputs(2, 4)
    m = build(cases.TINY_MOTION, dtype)
    y0 = m(x.to(DEV), 961, ctx.to(DEV)).sample.float()
    yz = m(x.to(DEV), 961, ctx.to(DEV), face_features=torch.zeros(256, 32, device=DEV, dtype=dtype)).sample.float()
    _same_function(yz, y0, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_shared_cfg_prefix_stays_on_with_face_features(dtype):
    """face_features alone keeps the shared prefix of a [uncond, cond] batch: the map is added ONCE to the half batch, in front of the
    duplication (the add runs on B / 2 * F * H * W rows), and the forward is the one without the prefix."""
    ops = _ops()
    x, ctx = cases.tiny_inputs(1, 4)
    x2 = x.repeat(2, 1, 1, 1, 1).to(DEV)
    ctx2 = torch.cat([ctx, seeded_randn(tuple(ctx.shape), 77)]).to(DEV)
    m = build(cases.TINY_MOTION, dtype)
    face = _face_rows(_controller(dtype)[0], _latent_mask(), dtype)
    y_plain = m(x2, 961, ctx2, face_features=face).sample.float()
    ops.PROFILER = ops.KernelProfiler()
    try:
        y_dup = m(x2, 961, ctx2, face_features=face, _halves_identical=True).sample.float()
        tags = [tag for (name, tag) in ops.PROFILER.by_shape() if name == "add_periodic"]
    finally:
        ops.PROFILER = None
    assert tags == [f"M={4 * 256} C=32 P=256"], tags
    assert float((y_plain - m(x2, 961, ctx2).sample.float()).abs().max()) > 1e-2
    if dtype == torch.float32:
        torch.testing.assert_close(y_dup, y_plain, rtol=1e-4, atol=1e-5)
    else:
        _same_function(y_dup, y_plain, dtype)


# =============================================================================== the loop
LOOP_KW = dict(num_inference_steps=3, guidance_scale=7.5, context_frames=16, context_stride=2, context_overlap=4, seed=0)
F_TOT = 20


def test_loop_geometry_has_a_wrapped_window():
    """the geometry of test_denoise_loop_wrapped_window_with_repeated_frames (CPU): three windows, two of them wrapped"""
    from emote_hack_amd.context import uniform
    wins = [list(map(int, c)) for c in uniform(0, LOOP_KW["num_inference_steps"], F_TOT, LOOP_KW["context_frames"], LOOP_KW["context_stride"],
                                               LOOP_KW["context_overlap"])]
    assert len(wins) >= 2 and all(len(w) == 16 for w in wins)
    assert any(any(b < a for a, b in zip(w, w[1:])) for w in wins), wins
    assert len({tuple(w) for w in wins}) == len(wins)


@pytest.fixture(scope="module")
def env():
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.conditioning import FaceLocator, SpeedEncoder
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    e = {}
    e["ref"] = build(cases.TINY, torch.float32, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    unet = build(cases.TINY_MOTION, torch.float32)
    ctl = _controller(torch.float32)[0]
    enc = SpeedEncoder(9, 128)
    enc.load_state_dict(synth_state_dict(enc.state_dict_shapes(), prefix="speed_encoder."))
    enc.to(DEV, torch.float32)
    loc = FaceLocator()
    lsd = synth_state_dict(loc.state_dict_shapes(), prefix="face_locator.")
    loc.load_state_dict(lsd)
    loc.to(DEV, torch.float32)
    g = torch.Generator().manual_seed(9)
    e["image"] = (torch.rand(128, 128, 3, generator=g) * 255).to(torch.uint8).numpy()
    # centre the synthetic locator's logits on this image, so that "logit > 0" is a mask with both classes (the bilinear upsampling
    # has unit weight sums: a bias shift is a logit shift)
    med = float(loc(torch.as_tensor(e["image"]).permute(2, 0, 1)[None].float().to(DEV) / 255.0).median())
    lsd["final_conv.bias"] = lsd["final_conv.bias"] - med
    loc.load_state_dict(lsd)
    loc.to(DEV, torch.float32)
    e["pipe"] = EMOAnimationPipeline(unet=unet, scheduler=DDIMScheduler(), speed_encoder=enc, face_region_controller=ctl, face_locator=loc)
    e["lat"], e["refl"], e["text"] = seeded_randn((1, 4, F_TOT, 16, 16), 5), seeded_randn((1, 4, 16, 16), 3), seeded_randn((2, 5, 32), 2)
    e["speeds"] = torch.tensor([cases.SPEEDS[i % len(cases.SPEEDS)] for i in range(F_TOT)])
    e["table"] = enc(e["speeds"])                                        # (F_tot, 4*C0) on the device
    mask = torch.zeros(128, 128, dtype=torch.bool)
    mask[20:90, 30:101] = True
    e["mask"] = mask
    e["cond"] = dict(speed_embeddings=e["table"][None], face_mask=mask)
    return e


def _denoise(e, lat=None, **kw):
    return e["pipe"].denoise((e["lat"] if lat is None else lat).to(DEV), e["refl"], e["text"], appearance_encoder=e["ref"], **dict(LOOP_KW, **kw))


@pytest.fixture(scope="module")
def eager(env):
    """the loop with both conditions, every kernel launched from Python"""
    return _denoise(env, use_graphs=False, **env["cond"])


def test_loop_graphs_on_is_graphs_off_and_the_conditions_are_live(env, eager):
    assert torch.equal(_denoise(env, use_graphs=True, **env["cond"]), eager)
    plain = _denoise(env, use_graphs=False)
    for one in ("speed_embeddings", "face_mask"):
        got = _denoise(env, use_graphs=False, **{one: env["cond"][one]})
        assert float((got - plain).abs().max()) > 1e-3 and float((got - eager).abs().max()) > 1e-3, one


def test_loop_equal_per_frame_speeds_are_the_one_speed_call(env):
    row = env["table"][3:4]
    one = _denoise(env, use_graphs=False, speed_embeddings=row)
    per_frame = _denoise(env, use_graphs=False, speed_embeddings=row.expand(F_TOT, -1).contiguous()[None])
    _same_function(per_frame, one, torch.float32)


def test_loop_step0_eps_is_the_window_average_of_hand_gathered_forwards(env):
    """Step 0 of the loop against direct UNet forwards: each window's latents AND speed rows gathered by hand with the window's frame
    list, the [uncond, cond] batch run through the UNet under the step's reference banks, the window average (one occurrence per frame,
    the last) and classifier-free guidance on the host.  A gather of the wrong frames' speed rows fails this."""
    pipe = env["pipe"]
    st = pipe.prepare_denoise(env["lat"].to(DEV), env["refl"], env["text"], appearance_encoder=env["ref"], use_graphs=False, return_eps=True,
                              **dict(LOOP_KW, **env["cond"]))
    assert len(st.windows) >= 2 and any(any(b < a for a, b in zip(w, w[1:])) for w in st.windows)
    pipe.denoise_step(st, 0)
    eps = st.eps_trace[0][0].cpu()
    x_in = env["lat"].to(DEV) * float(st.sched_frozen.input_scale(0))
    table = env["table"]
    acc, cnt = torch.zeros(2, 4, F_TOT, 16, 16), torch.zeros(F_TOT)
    for win in st.windows:
        ix = torch.tensor(win, device=DEV)
        x = x_in.index_select(2, ix)
        sp = table.index_select(0, ix)
        pipe.unet._reference_control = st.reader
        st.reader.set_projected_banks(st.kv_all[1], st.bank_idx, 1)
        y = pipe.unet(torch.cat([x, x]), st.t_buf, encoder_hidden_states=st.text, speed_embeddings=torch.stack([sp, sp]),
                      face_features=st.face_rows, return_dict=False)[0].cpu()
        for k, j in {k: j for j, k in enumerate(win)}.items():
            acc[:, :, k] += y[:, :, j]
            cnt[k] += 1
    assert bool((cnt > 0).all())
    u, c = acc[0] / cnt[None, :, None, None], acc[1] / cnt[None, :, None, None]
    torch.testing.assert_close(eps, u + LOOP_KW["guidance_scale"] * (c - u), rtol=1e-3, atol=1e-4)
    # the last window's forward with the speed rows of frames 0..15 instead of its own is another result: the check sees the gather
    wrong = table[:16]
    assert win != list(range(16))
    y_wrong = pipe.unet(torch.cat([x, x]), st.t_buf, encoder_hidden_states=st.text, speed_embeddings=torch.stack([wrong, wrong]),
                        face_features=st.face_rows, return_dict=False)[0].cpu()
    assert float((y_wrong - y).abs().max()) > 1e-3


def test_loop_reset_with_a_new_mask_and_new_speeds_is_a_fresh_prepare(env):
    pipe = env["pipe"]
    st = pipe.prepare_denoise(env["lat"].to(DEV), env["refl"], env["text"], appearance_encoder=env["ref"], use_graphs=True,
                              **dict(LOOP_KW, **env["cond"]))
    first = pipe._run_loop(st).clone()
    assert any(not isinstance(v, str) for v in st.graphs.values()), "the loop must have captured its graphs"
    lat2 = seeded_randn((1, 4, F_TOT, 16, 16), 15)
    mask2 = torch.zeros(16, 16)                                              # latent size this time
    mask2[2:9, 5:14] = 1.0
    table2 = env["table"].flip(0).contiguous()[None]
    pipe.reset_denoise(st, lat2.to(DEV), face_mask=mask2, speed_embeddings=table2)
    again = pipe._run_loop(st).clone()
    fresh = _denoise(env, lat=lat2, use_graphs=False, face_mask=mask2, speed_embeddings=table2)
    assert torch.equal(again, fresh) and not torch.equal(again, first)
    only_latents = _denoise(env, lat=lat2, use_graphs=False, **env["cond"])
    assert float((again - only_latents).abs().max()) > 1e-3                  # the new mask and speeds did enter
    st0 = pipe.prepare_denoise(env["lat"].to(DEV), env["refl"], env["text"], appearance_encoder=env["ref"], use_graphs=False, **LOOP_KW)
    with pytest.raises(ValueError, match="prepared without face_mask"):
        pipe.reset_denoise(st0, lat2.to(DEV), face_mask=mask2)
    with pytest.raises(ValueError, match="prepared without speed_embeddings"):
        pipe.reset_denoise(st0, lat2.to(DEV), speed_embeddings=table2)


# =============================================================================== __call__
def _call(e, **kw):
    return e["pipe"]("", video_length=F_TOT, height=128, width=128, latents=e["lat"].to(DEV), text_embeddings=e["text"], ref_image_latents=e["refl"],
                     output_type="latent", appearance_encoder=e["ref"], **dict(LOOP_KW, **kw)).videos


def test_call_locate_is_the_mask_computed_by_hand(env):
    loc = env["pipe"].face_locator
    logits = loc(torch.as_tensor(env["image"]).permute(2, 0, 1)[None].float().to(DEV) / 255.0)[0, 0]
    mask = logits > 0
    assert 0.05 < float(mask.float().mean()) < 0.95
    located = _call(env, face_mask="locate", source_image=env["image"])
    assert torch.equal(located, _call(env, face_mask=mask))
    assert float((located - _call(env)).abs().max()) > 1e-3


def test_call_head_speeds_per_frame_is_the_per_frame_speed_embeddings(env, eager):
    got = _call(env, head_speeds_per_frame=env["speeds"])
    assert torch.equal(got, _call(env, speed_embeddings=env["table"][None]))
    assert torch.equal(_call(env, head_speeds_per_frame=env["speeds"].tolist(), face_mask=env["mask"]), eager)
