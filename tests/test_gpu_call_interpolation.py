"""GPU tests of the pipeline call's tail: `__call__(interpolation_factor=, interpolation=, output_type="uint8")` - the frame
interpolation between the sampling loop and the VAE decode (EMOAnimationPipeline.py:824, :479-512) and the 8-bit output frames -
on the tiny UNet / ReferenceNet of the other `__call__` tests and the tiny VAE of tests/test_gpu_vae.py."""
import pytest
import torch

from emote_hack_amd.synth import seeded_randn
from tests import cases
from tests import interp_ref as R
from tests.test_gpu_kernels import DEV, ops
from tests.test_gpu_unet import build

pytestmark = pytest.mark.gpu
F_TOT = 16
LOOP_KW = dict(num_inference_steps=3, guidance_scale=7.5, context_frames=16, context_stride=1, context_overlap=4, seed=0)


@pytest.fixture(scope="module")
def env():
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    from tests.test_gpu_vae import SMALL, build as build_vae
    e = {}
    e["ref"] = build(cases.TINY, torch.float32, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    e["vae"] = build_vae(SMALL, torch.float32)[0]
    e["pipe"] = EMOAnimationPipeline(vae=e["vae"], unet=build(cases.TINY_MOTION, torch.float32), scheduler=DDIMScheduler())
    e["lat"], e["refl"], e["text"] = seeded_randn((1, 4, F_TOT, 16, 16), 5), seeded_randn((1, 4, 16, 16), 3), seeded_randn((2, 5, 32), 2)
    return e


def _call(e, output_type="latent", **kw):
    return e["pipe"]("", video_length=F_TOT, height=128, width=128, latents=e["lat"].to(DEV), text_embeddings=e["text"], ref_image_latents=e["refl"],
                     output_type=output_type, appearance_encoder=e["ref"], **dict(LOOP_KW, **kw)).videos


@pytest.fixture(scope="module")
def plain(env):
    """the latents of the call without any of the new keywords"""
    return _call(env)


def test_call_without_the_new_keywords_is_denoise_and_decode_video(env, plain):
    lat = env["pipe"].denoise(env["lat"].to(DEV), env["refl"], env["text"], appearance_encoder=env["ref"], **LOOP_KW)
    assert tuple(plain.shape) == (1, 4, F_TOT, 16, 16) and torch.equal(plain, lat)
    video = _call(env, output_type="tensor")
    assert video.dtype == torch.float32 and tuple(video.shape) == (1, 3, F_TOT, 128, 128)
    assert torch.equal(video, env["vae"].decode_video(lat))
    assert torch.equal(_call(env, interpolation_factor=1), plain)


def test_call_interpolation_factor_2_returns_the_interpolated_latents(env, plain):
    from emote_hack_amd import pipeline as P
    before = P.get_tensor_interpolation_method()
    got = _call(env, interpolation_factor=2)
    assert tuple(got.shape) == (1, 4, 2 * F_TOT - 1, 16, 16) and got.dtype == plain.dtype
    assert torch.equal(got[:, :, ::2], plain)
    assert torch.equal(got, ops().interpolate_frames(plain, 2, "slerp"))                 # None: slerp when no method was set
    assert bool(torch.isfinite(got).all())
    assert float((got[:, :, 1::2] - plain[:, :, :-1]).abs().max()) > 1e-3              # the odd frames are new frames
    assert P.get_tensor_interpolation_method() is before


def test_call_interpolation_linear_is_the_linear_restatement_and_leaves_the_global(env, plain):
    from emote_hack_amd import pipeline as P
    before = P.get_tensor_interpolation_method()
    try:
        P.set_tensor_interpolation_method(True)
        got = _call(env, interpolation_factor=2, interpolation="linear")
        assert P.get_tensor_interpolation_method() is P.slerp                            # the keyword is for this call only
        slerped = _call(env, interpolation_factor=2)
        assert torch.equal(slerped, _call(env, interpolation_factor=2, interpolation="slerp"))
        assert float((got - slerped).abs().max()) > 1e-4
        ref64, bound, e_ref = R.reference_and_bound(plain.cpu(), 2, "linear")
        err = float((R.generated(got.cpu().double(), 2) - R.generated(ref64, 2)).abs().max())
        print(f"call linear: kernel err {err:.3e}  e_ref {e_ref:.3e}  bound {bound:.3e}")
        assert err <= bound and torch.equal(got[:, :, ::2], plain)
        P.set_tensor_interpolation_method(False)                                         # None follows the method that was set
        assert torch.equal(_call(env, interpolation_factor=2), got)
    finally:
        P.tensor_interpolation = before


def test_call_output_type_uint8_decodes_the_interpolated_latents(env, plain):
    got = _call(env, output_type="uint8", interpolation_factor=2)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (1, 2 * F_TOT - 1, 128, 128, 3)
    lat2 = ops().interpolate_frames(plain, 2, "slerp")
    assert torch.equal(got, env["vae"].decode_video(lat2, output="uint8"))
    assert len(torch.unique(got)) > 16
    with pytest.raises(ValueError, match="video_length"):
        env["pipe"]("", video_length=1, height=128, width=128, latents=env["lat"][:, :, :1].to(DEV), text_embeddings=env["text"],
                    ref_image_latents=env["refl"], appearance_encoder=env["ref"], interpolation_factor=2, **LOOP_KW)
