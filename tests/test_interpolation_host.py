"""Host-side checks of the pipeline call's interpolation / 8-bit output keywords: bad values are refused before anything is allocated or
launched (so a stub pipeline without networks or a device reaches them), and `interpolate_latents` on CPU tensors stays the host path."""
import pytest
import torch

from emote_hack_amd.synth import seeded_randn
from tests import interp_ref as R


def _stub():
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd import pipeline as P
    return P.EMOAnimationPipeline(unet=type("U", (), {"device": torch.device("cpu")})(), scheduler=DDIMScheduler())


@pytest.mark.parametrize("kw,match", [
    (dict(interpolation_factor=0), "interpolation_factor"),
    (dict(interpolation_factor=2.5), "interpolation_factor"),
    (dict(interpolation_factor="2"), "interpolation_factor"),
    (dict(interpolation_factor=True), "interpolation_factor"),
    (dict(interpolation="cubic"), "interpolation="),
    (dict(interpolation_factor=2, video_length=1), "video_length"),
    (dict(interpolation_factor=3, video_length=None), "video_length"),
    (dict(output_type="uint8"), "VAE"),
])
def test_call_refuses_bad_interpolation_and_output_arguments(kw, match):
    pipe = _stub()
    kw = dict(dict(video_length=16), **kw)
    with pytest.raises(ValueError, match=match):
        pipe("", **kw)


def test_valid_keywords_pass_the_argument_checks():
    """a valid set goes on to the first thing the stub lacks (its UNet has no config): the checks themselves raise nothing"""
    pipe = _stub()
    for kw in (dict(interpolation_factor=2, interpolation="linear"), dict(interpolation_factor=1, interpolation="slerp", video_length=1), {}):
        with pytest.raises(AttributeError, match="config"):
            pipe("", **dict(dict(video_length=16), **kw))


def test_interpolate_latents_on_cpu_tensors_is_the_host_path():
    from emote_hack_amd import pipeline as P
    pipe = _stub()
    l3 = seeded_randn((1, 4, 3, 4, 4), 502)
    before = P.get_tensor_interpolation_method()
    try:
        P.tensor_interpolation = None
        with pytest.raises(TypeError, match="NoneType"):
            pipe.interpolate_latents(l3, 2, "cpu")
        assert pipe.interpolate_latents(l3, 1, "cpu") is l3
        for name, is_slerp in (("slerp", True), ("linear", False)):
            P.set_tensor_interpolation_method(is_slerp)
            assert torch.equal(pipe.interpolate_latents(l3, 3, "cpu"), R.interp(l3, 3, name, torch.float32))
        calls = []
        P.tensor_interpolation = lambda a, b, t: calls.append(t) or a              # a user-installed callable is called as before
        out = pipe.interpolate_latents(l3, 2, "cpu")
        assert calls == [0.5, 0.5] and torch.equal(out[:, :, 1], l3[:, :, 0])
    finally:
        P.tensor_interpolation = before
