"""The two weak conditions of the pipeline call - a face-region mask and per-frame head speeds - on the host: every argument check of
`__call__`, `reset_denoise` and the plan key, with stub models in the manner of tests/test_audio_io_host.py (the loop itself is
stubbed out: nothing is launched), the refusals of ControlNetModel / AppearanceEncoderModel, and the argument checks of the new kernel
entries, which the library makes before it launches anything (no GPU needed)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import cases
from tests.test_audio_io_host import StubSpeedEncoder, _pipe, _Stop

KW = dict(appearance_encoder=object(), ref_image_latents=torch.zeros(1, 4, 2, 2), latents=torch.zeros(1, 4, 2, 2, 2),
          text_embeddings=torch.zeros(2, 1, 5))        # video_length 2, a 2 x 2 latent = 16 x 16 pixels, C0 = 8


class StubController:
    def __init__(self, cin=1, cout=8):
        self.in_channels, self.out_channels = cin, cout


class StubLocator:
    def __init__(self):
        self.seen = []

    def __call__(self, images):
        self.seen.append(images)
        return images[:, :1] - 0.5       # "logits" (B, 1, H, W)


def test_ctor_takes_a_face_region_controller_and_a_face_locator():
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    unet = SimpleNamespace(device=torch.device("cpu"))
    p = EMOAnimationPipeline(unet=unet, scheduler=DDIMScheduler())
    assert p.face_region_controller is None and p.face_locator is None
    ctl, loc = StubController(), StubLocator()
    p = EMOAnimationPipeline(unet=unet, scheduler=DDIMScheduler(), face_region_controller=ctl, face_locator=loc)
    assert p.face_region_controller is ctl and p.face_locator is loc


def test_call_face_mask_argument_checks(monkeypatch):
    seen = {}
    p = _pipe(monkeypatch, seen)
    mask = torch.zeros(16, 16, dtype=torch.bool)
    with pytest.raises(ValueError, match="face_region_controller"):            # (the stub pipeline is built without __init__)
        p("", 2, face_mask=mask, **KW)
    p.face_region_controller = None
    with pytest.raises(ValueError, match="face_region_controller"):
        p("", 2, face_mask=mask, **KW)
    with pytest.raises(ValueError, match="face_region_controller"):            # ... whatever else is missing
        p("", 2, face_mask="locate", **KW)
    p.face_region_controller = StubController(1, 16)
    with pytest.raises(ValueError, match=r"FaceRegionController\(1, 8\)"):     # conv_in has 8 output channels
        p("", 2, face_mask=mask, **KW)
    p.face_region_controller = StubController(3, 8)
    with pytest.raises(ValueError, match=r"FaceRegionController\(1, 8\)"):
        p("", 2, face_mask=mask, **KW)
    p.face_region_controller = StubController(1, 8)
    for bad in (torch.zeros(8, 8), torch.zeros(16, 8), torch.zeros(1, 1, 4, 4), torch.zeros(2, 1, 16, 16), torch.zeros(16)):
        with pytest.raises(ValueError, match=r"pixel size \(16, 16\) or at latent size \(2, 2\)"):
            p("", 2, face_mask=bad, **KW)
    with pytest.raises(ValueError, match="locate"):
        p("", 2, face_mask="somewhere", **KW)
    for good in (mask, torch.ones(1, 1, 16, 16, dtype=torch.uint8), np.zeros((16, 16), np.float32), torch.rand(2, 2), torch.rand(1, 1, 2, 2)):
        seen.clear()
        with pytest.raises(_Stop):
            p("", 2, face_mask=good, **KW)
        assert seen["face_mask"] is good and seen["face_mask_threshold"] is None
    seen.clear()
    with pytest.raises(_Stop):                                                  # no mask: the loop is called as before
        p("", 2, **KW)
    assert seen["face_mask"] is None and seen["face_mask_threshold"] is None


def test_call_face_mask_locate(monkeypatch):
    seen = {}
    p = _pipe(monkeypatch, seen)
    p.face_region_controller = StubController(1, 8)
    img = np.zeros((16, 16, 3), np.uint8)
    img[4:8, :, 0] = 255
    with pytest.raises(ValueError, match="face_locator"):
        p("", 2, face_mask="locate", source_image=img, **KW)
    p.face_locator = StubLocator()
    with pytest.raises(ValueError, match="source_image"):
        p("", 2, face_mask="locate", **KW)
    assert not p.face_locator.seen
    with pytest.raises(_Stop):
        p("", 2, face_mask="locate", source_image=img, **KW)
    (fed,) = p.face_locator.seen
    assert fed.dtype == torch.float32 and tuple(fed.shape) == (1, 3, 16, 16) and float(fed.max()) == 1.0     # pixels in [0, 1]
    logits = seen["face_mask"]
    assert tuple(logits.shape) == (16, 16) and seen["face_mask_threshold"] == 0.0                              # sigmoid > 0.5
    assert torch.equal(logits > 0, torch.as_tensor(img[:, :, 0] > 0))


def test_call_head_speeds_per_frame_argument_checks(monkeypatch):
    seen = {}
    p = _pipe(monkeypatch, seen)
    with pytest.raises(ValueError, match="speed_encoder"):
        p("", 2, head_speeds_per_frame=[0.1, 0.2], **KW)
    p.speed_encoder = StubSpeedEncoder(64)
    with pytest.raises(ValueError, match=r"SpeedEncoder\(9, 32\)"):
        p("", 2, head_speeds_per_frame=[0.1, 0.2], **KW)
    p.speed_encoder = StubSpeedEncoder(32)
    with pytest.raises(ValueError, match="both name the head speed"):
        p("", 2, head_speeds_per_frame=[0.1, 0.2], head_rotation_speeds=0.3, **KW)
    for bad in ([0.1], [0.1, 0.2, 0.3], 0.5):
        with pytest.raises(ValueError, match=rf"got {np.size(bad)} values for video_length 2"):
            p("", 2, head_speeds_per_frame=bad, **KW)
    assert not p.speed_encoder.seen
    for v in ([0.1, -0.2], torch.tensor([0.1, -0.2]), np.array([[0.1], [-0.2]])):
        seen.clear()
        with pytest.raises(_Stop):
            p("", 2, head_speeds_per_frame=v, **KW)
        arg = p.speed_encoder.seen[-1]
        assert arg.dtype == torch.float32 and tuple(arg.shape) == (2,)                # ONE encoder call over the clip's frames
        se = seen["speed_embeddings"]
        assert tuple(se.shape) == (1, 2, 32) and torch.equal(se[0, :, 0], torch.tensor([0.1, -0.2]))
    n = len(p.speed_encoder.seen)
    assert n == 3
    # head_rotation_speeds= keeps its contract: ONE speed per clip, one shared (1, 4*C0) row
    with pytest.raises(ValueError, match="ONE speed per clip"):
        p("", 2, head_rotation_speeds=[0.1, 0.2], **KW)
    with pytest.raises(_Stop):
        p("", 2, head_rotation_speeds=0.3, **KW)
    assert tuple(seen["speed_embeddings"].shape) == (1, 32)
    # an explicit speed_embeddings= takes precedence: the encoder is not called
    n = len(p.speed_encoder.seen)
    given = torch.zeros(1, 2, 32)
    with pytest.raises(_Stop):
        p("", 2, head_speeds_per_frame=[0.1, 0.2], speed_embeddings=given, **KW)
    assert len(p.speed_encoder.seen) == n and seen["speed_embeddings"] is given


def test_call_speed_embeddings_forms(monkeypatch):
    seen = {}
    p = _pipe(monkeypatch, seen)
    for good in (torch.zeros(1, 32), torch.zeros(2, 32), torch.zeros(1, 2, 32), torch.zeros(2, 2, 32)):
        with pytest.raises(_Stop):
            p("", 2, speed_embeddings=good, **KW)
        assert seen["speed_embeddings"] is good
    with pytest.raises(ValueError, match="hold 3 frames, the clip has 2"):
        p("", 2, speed_embeddings=torch.zeros(1, 3, 32), **KW)
    with pytest.raises(ValueError, match="hold 1 frames, the clip has 2"):
        p("", 2, speed_embeddings=torch.zeros(2, 1, 32), **KW)
    for bad in (torch.zeros(3, 32), torch.zeros(3, 2, 32), torch.zeros(32), torch.zeros(1, 1, 2, 32)):
        with pytest.raises(ValueError, match="1 row"):
            p("", 2, speed_embeddings=bad, **KW)


def _state(**kw):
    """what `_bind_inputs` reads of a prepared state, for a 2-frame clip of 2 x 2 latents on the CPU"""
    st = SimpleNamespace(latents=torch.zeros(1, 4, 2, 2, 2), side=None, n_ref_images=1, C4=4, h=2, w=2, cfg=True, calls=[], audio_features=None,
                         speed=None, face_rows=None, controlnet=None, graphs={}, bank_variants=[], plans={})
    st.__dict__.update(kw)
    return st


def test_reset_denoise_takes_the_inputs_a_state_was_prepared_with_and_refuses_the_others(monkeypatch):
    p = _pipe(monkeypatch, {})
    p.face_region_controller = StubController(1, 8)
    lat = torch.ones(1, 4, 2, 2, 2)
    with pytest.raises(ValueError, match="prepared without face_mask"):
        p.reset_denoise(_state(), lat, face_mask=torch.zeros(16, 16))
    with pytest.raises(ValueError, match="prepared without speed_embeddings"):
        p.reset_denoise(_state(), lat, speed_embeddings=torch.zeros(1, 2, 32))
    with pytest.raises(ValueError, match="prepared with per-clip speed_embeddings"):
        p.reset_denoise(_state(speed=torch.zeros(1, 32)), lat, speed_embeddings=torch.zeros(1, 2, 32))
    with pytest.raises(ValueError, match="prepared with per-frame speed_embeddings"):
        p.reset_denoise(_state(speed=torch.zeros(1, 2, 32)), lat, speed_embeddings=torch.zeros(1, 32))
    with pytest.raises(ValueError, match="speed_embeddings"):                          # [uncond, cond] for a state with one shared table
        p.reset_denoise(_state(speed=torch.zeros(1, 2, 32)), lat, speed_embeddings=torch.zeros(2, 2, 32))
    st = _state(speed=torch.zeros(1, 2, 32))
    new = torch.arange(64.0).reshape(1, 2, 32)
    p.reset_denoise(st, lat, speed_embeddings=new)
    assert torch.equal(st.speed, new) and torch.equal(st.latents, lat)
    # a mask of the wrong size is refused before the controller runs, for a state that has the buffer
    with pytest.raises(ValueError, match=r"pixel size \(16, 16\)"):
        p.reset_denoise(_state(face_rows=torch.zeros(4, 8)), lat, face_mask=torch.zeros(8, 8))


def test_plan_key_sees_presence_and_shapes(monkeypatch):
    from emote_hack_amd import DDIMScheduler
    p = _pipe(monkeypatch, {})
    p.scheduler = DDIMScheduler()
    lat, ref, text = KW["latents"], KW["ref_image_latents"], KW["text_embeddings"]
    key = lambda **kw: p._plan_key(lat, ref, text, kw)
    base = key()
    assert key(face_mask=None, face_mask_threshold=None) == base
    masked = key(face_mask=torch.zeros(16, 16))
    assert masked != base
    assert key(face_mask=torch.ones(2, 2), face_mask_threshold=0.0) == masked           # another mask, another size: the same plan
    per_clip, per_frame = key(speed_embeddings=torch.zeros(1, 32)), key(speed_embeddings=torch.zeros(1, 2, 32))
    assert len({base, per_clip, per_frame, key(speed_embeddings=torch.zeros(2, 2, 32))}) == 4
    assert key(speed_embeddings=torch.ones(1, 2, 32)) == per_frame


def test_reference_net_and_controlnet_refuse_per_frame_speed_embeddings():
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.controlnet import ControlNetModel
    x, ctx = torch.zeros(1, 4, 16, 16), torch.zeros(1, 5, 32)
    with pytest.raises(ValueError, match="AppearanceEncoderModel takes speed_embeddings"):
        AppearanceEncoderModel(**cases.TINY)(x, 1, ctx, speed_embeddings=torch.zeros(1, 1, 128))
    with pytest.raises(ValueError, match="ControlNetModel takes speed_embeddings"):
        ControlNetModel(**cases.TINY)(x, 1, ctx, None, speed_embeddings=torch.zeros(1, 1, 128))


# ------------------------------------------------------------------------------- the entries' own argument checks (made before any launch)
def _lib():
    from emote_hack_amd import _lib as L
    return L.load()


def test_add_periodic_and_mask_pool_refusals_need_no_gpu():
    lib = _lib()
    a = 4096            # a non-NULL, 16-byte aligned address that is never dereferenced: every call below is refused
    add = lambda M, Cc, P, ld=None, dt=0, x=a, f=a, y=a: lib.emo_add_periodic(x, ld or Cc, f, ld or Cc, y, ld or Cc, M, Cc, P, dt, None)
    assert add(28, 8, 8) != 0 and b"whole number of periods" in lib.emo_last_error_string()      # M % P != 0
    assert add(28, 8, 0) != 0 and add(0, 8, 7) != 0
    assert add(28, 6, 7) != 0 and add(28, 12, 7, dt=1) != 0                                       # C not a multiple of the vector
    assert add(28, 8, 7, ld=4) != 0                                                               # rows narrower than C
    assert add(28, 8, 7, x=None) != 0 and add(28, 8, 7, f=a + 4) != 0 and add(28, 8, 7, dt=7) != 0
    pool = lambda Hp, Wp, dt=0, x=a, y=a: lib.emo_mask_pool(x, y, Hp, Wp, 0, 0.0, dt, None)
    assert pool(12, 24) != 0 and b"multiples of 8" in lib.emo_last_error_string()
    assert pool(16, 20) != 0 and pool(0, 8) != 0 and pool(16, 24, x=None) != 0 and pool(16, 24, x=a + 4) != 0 and pool(16, 24, dt=3) != 0


def test_groupnorm_mod_rows_refusals_need_no_gpu():
    lib = _lib()
    a = 4096
    N, S, Cc, G = 2, 15, 16, 4
    one = lambda mod_rows, mod=a, ld=2 * Cc: lib.emo_groupnorm_mod_rows(a, Cc, a, a, mod, ld, mod_rows, a, Cc, N, S, Cc, G, 1e-5, 0, 0, None)
    two = lambda mod_rows, mod=a, ld=2 * Cc: lib.emo_groupnorm_apply_mod_rows(a, Cc, a, a, a, mod, ld, mod_rows, a, Cc, N, S, Cc, G, 1e-5, 0, 0, None)
    tab = lambda mod_rows, mod=a, ld=2 * Cc: lib.emo_groupnorm_coeffs_mod_rows(a, a, a, mod, ld, mod_rows, a, N, S, Cc, G, 1e-5, 0, None)
    for call in (one, two, tab):
        assert call(4) != 0 and b"must divide" in lib.emo_last_error_string()         # a frame would straddle two instances
        assert call(0) != 0 and call(-5) != 0 and call(30) != 0
        assert call(5, mod=None) != 0 and call(5, mod=a + 4) != 0 and call(5, ld=2 * Cc - 4) != 0 and call(5, ld=2 * Cc + 2) != 0
