"""emote_hack_amd - MI355X-native diffusion hot path of johndpope/Emote-hack.

Host-side mirror of the reference's Python surface for that path (UNet3DConditionModel,
ReferenceAttentionControl, EMOAnimationPipeline, schedulers, context windows) over hand-written
gfx950 HIP kernels reached through the C ABI in include/emo_hip.h.  No CPU fallback.
"""
from .config import normalize_unet_config, unet_config_from_yaml  # noqa: F401
from .context import get_context_scheduler, ordered_halving, uniform  # noqa: F401
from .scheduler import (DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler,  # noqa: F401
                        EulerDiscreteScheduler, LMSDiscreteScheduler)


def __getattr__(name):  # heavy modules on demand
    if name in ("UNet3DConditionModel", "UNet3DConditionOutput"):
        from . import unet
        return getattr(unet, name)
    if name == "ReferenceAttentionControl":
        from .reference_control import ReferenceAttentionControl
        return ReferenceAttentionControl
    if name in ("EMOAnimationPipeline", "AnimationPipelineOutput"):
        from . import pipeline
        return getattr(pipeline, name)
    if name in ("ControlNetModel", "ControlNetOutput"):
        from . import controlnet
        return getattr(controlnet, name)
    if name in ("CLIPTextModel", "clip_text_param_shapes", "clip_text_synth_state_dict"):
        from . import clip_text
        return getattr(clip_text, name)
    if name in ("CLIPVisionModel", "CLIPVisionModelWithProjection", "CLIPImageProcessor", "clip_vision_param_shapes",
                "clip_vision_synth_state_dict"):
        from . import clip_vision
        return getattr(clip_vision, name)
    if name in ("save_videos_grid", "images2video", "video2images", "encode_mjpeg", "write_avi", "read_avi", "jpeg_tables",
                "save_images_grid", "encode_png", "encode_apng", "write_png", "write_apng", "parse_png", "decode_png", "decode_apng", "parse_gif", "decode_gif",
                "read_image", "read_video"):
        from . import video_io
        return getattr(video_io, name)
    if name == "AppearanceEncoderModel":
        from .appearance_encoder import AppearanceEncoderModel
        return AppearanceEncoderModel
    raise AttributeError(name)
