"""GPU checks of the wav2vec2-large family (feat_extract_norm "layer", conv biases, pre-LN encoder, attention_mask): the two kernels
behind its feature encoder - emo_layernorm_act and emo_wav_conv0_ln_act - against float64 restatements at the TOL table of
tests/test_gpu_kernels.py, and the model against the outputs of transformers' own Wav2Vec2Model on the same name-keyed weights and
seeded waveforms (tests/golden/wav2vec2_large.safetensors, tools/oracle/gen_golden_wav2vec2_large.py).  f32 mode at rtol 1e-3 /
atol 1e-4; bf16 / fp16 against transformers' OWN low-precision error for the same input (recorded in the .json): mean error <= 1.25x,
max error <= 2x - the rule of the yard-stick branch of tests/test_gpu_unet.py::check."""
import ctypes as C
import json

import pytest
import torch
import torch.nn.functional as F
from safetensors.torch import load_file

from emote_hack_amd import ops
from emote_hack_amd.synth import seeded_randn
from tests import cases
from tests import wav2vec2_large_cases as L
from tests.test_gpu_kernels import DEV, DTYPES, TOL

pytestmark = pytest.mark.gpu
IDS = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
SENTINEL = 3.0          # fills the columns beside a strided view (exact in every dtype)
EPS = 1e-5


def within(label, got, ref64, dtype):
    """the assert_close condition |got - ref| <= atol + rtol * |ref| of TOL[dtype], evaluated where the tensors live"""
    tol = TOL[dtype]
    g = got.double()
    assert g.shape == ref64.shape and bool(torch.isfinite(g).all()), (label, "shape / not finite")
    worst = float(((g - ref64).abs() / (tol["atol"] + tol["rtol"] * ref64.abs())).max())
    print(f"{label}: worst error / tolerance {worst:.3f}")
    assert worst <= 1.0, (label, worst)


def affine(Cc, seed):
    return (1 + 0.2 * seeded_randn((Cc,), seed)).to(DEV), (0.2 * seeded_randn((Cc,), seed + 1)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------- emo_layernorm_act
def second_trip_rows(Cc, dtype):
    """the smallest M whose rows need a second trip of the capped grid, from the library's own plan"""
    from emote_hack_amd import _lib
    plan = (C.c_int * 4)()
    assert _lib.load().emo_layernorm_plan(1, Cc, ops.dt(dtype), plan) == 0
    M = 4096 * 4 * plan[1] + 3
    assert _lib.load().emo_layernorm_plan(M, Cc, ops.dt(dtype), plan) == 0 and plan[3] == 1 and plan[2] == 4096
    return M


def ln_act_case(M, Cc, dtype, pad, fill=SENTINEL):
    x = torch.full((M, Cc + pad), SENTINEL, dtype=dtype, device=DEV)
    x[:, :Cc] = (1.5 * torch.randn(M, Cc, device=DEV, generator=torch.Generator(DEV).manual_seed(M + Cc)) + 0.3).to(dtype)
    y = torch.full((M, Cc + 2 * pad), fill, dtype=dtype, device=DEV)
    return x, y


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("Cc", [32, 40, 512, 1024])
def test_layernorm_act_vs_float64(Cc, dtype):
    """1 lane per row (32), a vector count that is no power of two (40), many lanes (512, 1024); M = 1, a ragged last row group, several
    blocks; strided input and output whose other columns come back untouched; GELU on and off"""
    g, b = affine(Cc, 11)
    for M in (1, 63, 799):
        x, y = ln_act_case(M, Cc, dtype, 8)
        for gelu in (True, False):
            y.fill_(SENTINEL)
            out = ops.layer_norm_act(x[:, :Cc], g, b, EPS, gelu=gelu, out=y[:, :Cc])
            assert out.data_ptr() == y.data_ptr()
            ref = F.layer_norm(x[:, :Cc].double(), (Cc,), g.double(), b.double(), EPS)
            within(f"layernorm_act M={M} C={Cc} {IDS[dtype]} gelu={gelu}", y[:, :Cc], F.gelu(ref) if gelu else ref, dtype)
            assert bool((y[:, Cc:] == SENTINEL).all()) and bool((x[:, Cc:] == SENTINEL).all())
        # act = 0 is emo_layernorm(pe = NULL), bit for bit
        assert torch.equal(ops.layer_norm_act(x[:, :Cc], g, b, EPS, gelu=False), ops.layer_norm(x[:, :Cc], g, b, EPS))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_layernorm_act_second_grid_trip(dtype):
    """rows past the grid cap: every row of a NaN-filled output is written, and written right"""
    Cc = 1024
    M = second_trip_rows(Cc, dtype)
    g, b = affine(Cc, 13)
    x, y = ln_act_case(M, Cc, dtype, 0, fill=float("nan"))
    ops.layer_norm_act(x, g, b, EPS, gelu=True, out=y)
    within(f"layernorm_act second trip M={M} {IDS[dtype]}", y, F.gelu(F.layer_norm(x.double(), (Cc,), g.double(), b.double(), EPS)), dtype)
    assert torch.equal(ops.layer_norm_act(x, g, b, EPS, gelu=False), ops.layer_norm(x, g, b, EPS))


# ------------------------------------------------------------------------------------------------------------- emo_wav_conv0_ln_act
def conv0_operands(Cc, k, n):
    w = (seeded_randn((Cc, k), 21) / k ** 0.5).to(DEV)
    bias = (0.3 * seeded_randn((Cc,), 22)).to(DEV)
    wave = (seeded_randn((n,), 23 + n) + 0.2).to(DEV)
    return wave, w, bias


def conv0_ref64(wave, w, bias, g, b, stride):
    """float64 conv1d + bias (as a product with the window matrix) -> layer_norm -> gelu, on the device"""
    pre = wave.double().unfold(0, w.shape[1], stride) @ w.double().t() + bias.double()
    return F.gelu(F.layer_norm(pre, (w.shape[0],), g.double(), b.double(), EPS))


@pytest.mark.parametrize("Cc,k,stride", [(32, 10, 5), (512, 10, 5), (40, 3, 2), (1024, 16, 1)], ids=lambda v: str(v))
def test_wav_conv0_ln_act_vs_float64(Cc, k, stride):
    """one row, still one row, two rows, odd remainders, 3 s of audio; 8 lanes per row, 64, a vector count that is no power of two, two
    vectors per lane; all three output dtypes into a strided output against ONE float64 reference (the weights stay f32), and in f32 the
    window-matrix GEMM + emo_layernorm_act route as well"""
    g, b = affine(Cc, 31)
    for n in (k, k + stride - 1, k + stride, 4001, 48000):
        wave, w, bias = conv0_operands(Cc, k, n)
        T0 = (n - k) // stride + 1
        ref = conv0_ref64(wave, w, bias, g, b, stride)
        assert ref.shape == (T0, Cc)
        for dtype in DTYPES:
            y = torch.full((T0, Cc + 8), SENTINEL, dtype=dtype, device=DEV)
            ops.wav_conv0_ln_act(wave, w, bias, g, b, stride, EPS, gelu=True, dtype=dtype, out=y[:, :Cc])
            within(f"wav_conv0 C={Cc} k={k} s={stride} n={n} {IDS[dtype]}", y[:, :Cc], ref, dtype)
            assert bool((y[:, Cc:] == SENTINEL).all())
        kp = (k + 7) // 8 * 8
        a0 = F.pad(wave.unfold(0, k, stride), (0, kp - k)).contiguous().view(-1).view(T0, kp)       # (one row: a row stride of kp, not of the unfold)
        via_gemm = ops.layer_norm_act(ops.gemm(a0, F.pad(w, (0, kp - k)).contiguous(), bias), g, b, EPS, gelu=True)
        within(f"wav_conv0 C={Cc} k={k} s={stride} n={n} GEMM route", via_gemm, ref, torch.float32)
        fused = ops.wav_conv0_ln_act(wave, w, bias, g, b, stride, EPS, gelu=True, dtype=torch.float32)
        within(f"wav_conv0 C={Cc} k={k} s={stride} n={n} fused vs GEMM route", fused, via_gemm.double(), torch.float32)
    plain = ops.wav_conv0_ln_act(wave, w, bias, g, b, stride, EPS, gelu=False, dtype=torch.float32)        # act = 0
    pre = wave.double().unfold(0, k, stride) @ w.double().t() + bias.double()
    within(f"wav_conv0 C={Cc} no act", plain, F.layer_norm(pre, (Cc,), g.double(), b.double(), EPS), torch.float32)


@pytest.mark.parametrize("Cc,k,stride,n", [(36, 10, 5, 4000), (1032, 10, 5, 4000), (512, 17, 5, 4000), (512, 10, 5, 9)])
def test_wav_conv0_ln_act_refusals_leave_the_output_untouched(Cc, k, stride, n):
    from emote_hack_amd._lib import EmoHipError
    g, b = affine(Cc, 31)
    wave, w, bias = conv0_operands(Cc, k, n)
    y = torch.full((max((n - k) // stride + 1, 1), Cc), SENTINEL, device=DEV)
    assert not ops.wav_conv0_ln_act_ok(n, Cc, k, stride)
    with pytest.raises(EmoHipError, match=r"emo_status -3"):
        ops.wav_conv0_ln_act(wave, w, bias, g, b, stride, EPS, out=y)
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def gold():
    return load_file(L.GOLDEN)


@pytest.fixture(scope="module")
def meta():
    with open(L.GOLDEN_JSON) as f:
        return json.load(f)


def _model(cfg, dtype=torch.float32):
    from emote_hack_amd.wav2vec2 import Wav2Vec2Model, wav2vec2_synth_state_dict
    m = Wav2Vec2Model(cfg)
    m.load_state_dict(wav2vec2_synth_state_dict(cfg))
    return m.to(DEV, dtype)


@pytest.fixture(scope="module")
def tiny_large():
    return _model(L.TINY_LARGE)


@pytest.fixture(scope="module")
def wide():
    return _model(L.WIDE)


def close32(got, want):
    torch.testing.assert_close(got.cpu(), want, rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("route", ["fused", "gemm"])
def test_tiny_large_goldens_f32(gold, tiny_large, route):
    for n in L.LENGTHS:
        close32(tiny_large(L.wave(n), conv0_route=route).last_hidden_state, gold[f"tiny_large/out_{n}"])
    for norm, stable in L.COMBOS:
        m = _model(L.combo_config(norm, stable))
        m.conv0_route = route           # the attribute selects the route as the keyword does
        close32(m(L.wave(L.COMBO_N)).last_hidden_state, gold[L.combo_key(norm, stable)])


def test_conv0_routes_agree_and_fall_back(gold):
    """a first layer the fused kernel does not serve (k = 20) takes the GEMM route whatever is asked for"""
    cfg = dict(L.TINY_LARGE, conv_kernel=(20, 3, 3, 3, 3, 2, 2))
    m = _model(cfg)
    x = L.wave(4000)
    assert not ops.wav_conv0_ln_act_ok(4000, 32, 20, 5)
    assert torch.equal(m(x, conv0_route="fused").last_hidden_state, m(x, conv0_route="gemm").last_hidden_state)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_wide_vs_transformers_golden(gold, meta, wide, dtype):
    """LARGE_CONFIG's widths at depth 4 on 1 s of audio -> (1, 49, 1024)"""
    iv = load_file(cases.GOLDEN_DIR + "/wav2vec2.safetensors")["base/input_values"]
    y = wide.to(DEV, dtype)(iv).last_hidden_state.cpu()
    assert y.shape == (1, 49, 1024) and y.dtype == torch.float32
    if dtype == torch.float32:
        close32(y, gold["wide/out"])
        return
    name = "bf16" if dtype == torch.bfloat16 else "fp16"
    yard = meta["low_precision_error"]["wide"][name]
    theirs = (gold[f"wide/out_{name}"].float() - gold["wide/out"]).abs()
    assert abs(float(theirs.mean()) - yard["mean"]) <= 1e-6 and abs(float(theirs.max()) - yard["max"]) <= 1e-6      # the record is of these tensors
    e = (y - gold["wide/out"]).abs()
    print(f"wav2vec2 wide {name}: HIP mean err {float(e.mean()):.3e} max {float(e.max()):.3e}; "
          f"transformers' own: mean {yard['mean']:.3e} max {yard['max']:.3e}")
    assert float(e.mean()) <= 1.25 * yard["mean"] and float(e.max()) <= 2.0 * yard["max"]


def test_padded_batch_with_attention_mask(gold, tiny_large):
    iv = gold["tiny_large/batch_input_values"]
    n0, n1 = L.BATCH_LENGTHS
    t0, t1 = L.BATCH_FRAMES
    mask = torch.zeros(2, n0, dtype=torch.long)
    mask[0], mask[1, :n1] = 1, 1
    y = tiny_large(iv, attention_mask=mask).last_hidden_state
    assert y.shape == (2, t0, 64)
    close32(y[0, :t0], gold["tiny_large/batch_out_0"])
    close32(y[1, :t1], gold["tiny_large/batch_out_1"])
    assert bool((y[1, t1:] == 0).all())
    # each utterance is the utterance run alone, exactly
    assert torch.equal(y[0], tiny_large(iv[:1]).last_hidden_state[0])
    assert torch.equal(y[1, :t1], tiny_large(iv[1:, :n1]).last_hidden_state[0])
    # an all-ones mask is no mask; a batch without a mask is its rows
    both = tiny_large(iv).last_hidden_state
    assert torch.equal(tiny_large(iv, attention_mask=torch.ones(2, n0)).last_hidden_state, both)
    assert torch.equal(both[0], y[0]) and torch.equal(both[1], tiny_large(iv[1:]).last_hidden_state[0])
    assert torch.equal(tiny_large(iv.to(DEV), attention_mask=mask.to(DEV)).last_hidden_state, y)


def test_base_family_is_where_it_was():
    """the shared feature-encoder and positional-conv code did not move the group-norm, post-LN family"""
    base = load_file(cases.GOLDEN_DIR + "/wav2vec2.safetensors")
    y = _model(cases.WAV2VEC2_TINY)(0.5 * seeded_randn((1, 4000), 501)).last_hidden_state
    close32(y, base["tiny/out"])


def test_pipeline_call_takes_a_large_family_extractor(tiny_large):
    """EMOAnimationPipeline.__call__(audio=waveform, feature_extractor=Wav2VecFeatureExtractor(<layer-norm family model>)): the context
    width follows the model's hidden size (64 here, 1024 for LARGE_CONFIG) with no change to the extractor or the pipeline - same
    latents as passing the audio_features= built from extract_features."""
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.conditioning import audio_context_tokens
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    from emote_hack_amd.wav2vec2 import Wav2VecFeatureExtractor
    from tests.test_gpu_unet import build
    cfg = dict(cases.TINY_MOTION, cross_attention_dim=64)
    unet = build(cfg, torch.float32)
    ref = build(dict(cases.TINY, cross_attention_dim=64), torch.float32, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    fx = Wav2VecFeatureExtractor(tiny_large, DEV)
    wave = 0.5 * seeded_randn((4000,), 501)
    pipe = EMOAnimationPipeline(unet=unet, scheduler=DDIMScheduler())
    kw = dict(video_length=4, height=128, width=128, num_inference_steps=2, guidance_scale=7.5, context_frames=4, context_stride=1,
              context_overlap=0, output_type="latent", appearance_encoder=ref, text_embeddings=seeded_randn((2, 5, 64), 2),
              ref_image_latents=seeded_randn((1, 4, 16, 16), 3), latents=seeded_randn((1, 4, 4, 16, 16), 1).to(DEV), seed=0)
    a = pipe("", audio=wave, feature_extractor=fx, **kw).videos
    feats = audio_context_tokens(fx.extract_features(wave), 4, 64)
    assert feats.shape == (4, 5, 64)
    b = pipe("", audio_features=feats, **kw).videos
    assert torch.equal(a, b)
    c = pipe("", **kw).videos
    assert float((a - c).abs().max()) > 1e-4          # the audio context is live
