"""EMOAnimationPipeline - the sampling loop of the reference (EMOAnimationPipeline.py:543-840) on
MI355X.  Same `__call__` signature; the hot loop (`:698-823`) is re-designed and lives in emote_hack_amd/denoise_loop.py (DenoiseLoop, the
base class: prepare_denoise, denoise_step, denoise, reset_denoise, denoise_chained); this module keeps the reference-named surface.

Prompts are encoded by `_encode_prompt` (:202-289) with the caller's tokenizer and a text encoder on the pipeline - on these kernels
emote_hack_amd.clip_text.CLIPTextModel; `text_embeddings=` still takes precedence.
Caller-supplied where out of scope: VAE (`vae=` object with encode / decode_video, see emote_hack_amd/vae.py),
wav2vec (`audio_features=`, windowed by emote_hack_amd.conditioning.audio_windows), `speed_embeddings=`.
"""
from __future__ import annotations

import logging
import math
import numbers
import os
from dataclasses import dataclass
from fractions import Fraction
from typing import Callable, List, Optional, Union

import torch

from . import ops
from .denoise_loop import DenoiseLoop

logger = logging.getLogger(__name__)


@dataclass
class AnimationPipelineOutput:  # EMOAnimationPipeline.py:79-81
    videos: Union[torch.Tensor, "object"]


# ---- magicanimate/utils/util.py:116-140 (the frame interpolation `interpolate_latents` uses)
tensor_interpolation = None


def get_tensor_interpolation_method():
    return tensor_interpolation


def set_tensor_interpolation_method(is_slerp):
    global tensor_interpolation
    tensor_interpolation = slerp if is_slerp else linear


def linear(v1, v2, t):
    return (1.0 - t) * v1 + t * v2


def slerp(v0: torch.Tensor, v1: torch.Tensor, t: float, DOT_THRESHOLD: float = 0.9995) -> torch.Tensor:
    """spherical interpolation of two tensors taken as single vectors; linear when they are nearly parallel (util.py:128-140)"""
    dot = ((v0 / v0.norm()) * (v1 / v1.norm())).sum()
    if dot.abs() > DOT_THRESHOLD:
        return (1.0 - t) * v0 + t * v1
    omega = dot.acos()
    return (((1.0 - t) * omega).sin() * v0 + (t * omega).sin() * v1) / omega.sin()


class EMOAnimationPipeline(DenoiseLoop):
    def __init__(self, vae=None, text_encoder=None, tokenizer=None, unet=None, controlnet=None, scheduler=None, image_encoder=None,
                 image_processor=None, speed_encoder=None, face_region_controller=None, face_locator=None):
        """EMOAnimationPipeline.py:87-130.  The ctor forces steps_offset=1 / clip_sample=False on the
        scheduler it is given, like the reference.  image_encoder= (the reference's ctor call, :909-917) is a
        CLIPVisionModelWithProjection - on these kernels emote_hack_amd.clip_vision's; image_processor= defaults to that module's
        CLIPImageProcessor at the encoder's image_size.  speed_encoder= is an emote_hack_amd.conditioning.SpeedEncoder for
        `__call__(head_rotation_speeds=)` / `__call__(head_speeds_per_frame=)`; face_region_controller= an
        emote_hack_amd.conditioning.FaceRegionController(1, block_out_channels[0]) for `face_mask=` and face_locator= an
        emote_hack_amd.conditioning.FaceLocator for `face_mask="locate"`; the three attributes may also be assigned afterwards."""
        if unet is None or scheduler is None:
            raise ValueError("unet and scheduler are required")
        if not hasattr(scheduler, "step_plan"):
            # PNDM (51 UNet evaluations for 50 steps, a repeated timestep restarting from an earlier sample) among others: the
            # loop's step / window / ReferenceNet-group bookkeeping assumes one UNet evaluation per step
            raise TypeError(f"{type(scheduler).__name__} is not served: the loop runs DDIMScheduler, DDPMScheduler, "
                            "DPMSolverMultistepScheduler, EulerDiscreteScheduler, EulerAncestralDiscreteScheduler, LMSDiscreteScheduler "
                            "(or an object with their `step_plan(si, first)` interface)")
        self.vae, self.text_encoder, self.tokenizer = vae, text_encoder, tokenizer
        self.unet, self.controlnet, self.scheduler = unet, controlnet, scheduler
        if image_encoder is not None and image_processor is None:
            from .clip_vision import CLIPImageProcessor
            S = image_encoder.config.image_size
            image_processor = CLIPImageProcessor(size={"shortest_edge": S}, crop_size={"height": S, "width": S},
                                                 device=getattr(image_encoder, "device", unet.device))
        self.image_encoder, self.image_processor = image_encoder, image_processor
        self.speed_encoder = speed_encoder
        self.face_region_controller, self.face_locator = face_region_controller, face_locator
        # EMOAnimationPipeline.py:105-117: ANY scheduler whose config has the key, not DDIM only - a DDPMScheduler handed to the
        # pipeline runs [981, ..., 1] on 50 of 1000 steps, like a diffusers DDPMScheduler would under the reference ctor
        if getattr(scheduler.config, "steps_offset", 1) != 1:
            scheduler.config.steps_offset = 1
        if getattr(scheduler.config, "clip_sample", False):
            scheduler.config.clip_sample = False
        self.vae_scale_factor = 8
        self.device = unet.device
        self._plan_cache = None   # (plan key, prepared state) of the last `denoise(reuse_state=True)` / `__call__`

    @property
    def _execution_device(self):
        return self.unet.device

    def check_inputs(self, prompt, height, width, callback_steps):  # EMOAnimationPipeline.py:326-339
        if not isinstance(prompt, str) and not isinstance(prompt, list):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if (callback_steps is None) or (not isinstance(callback_steps, int) or callback_steps <= 0):
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps} of type {type(callback_steps)}.")

    @torch.no_grad()
    def _encode_prompt(self, prompt, device, num_videos_per_prompt, do_classifier_free_guidance, negative_prompt):
        """EMOAnimationPipeline.py:202-289: tokenize (max_length padding, truncation with a warning), encode, [uncond, cond] under
        classifier-free guidance.  The two halves go through ONE text-encoder call (the ids are stacked; every sequence is encoded
        on its own, so this equals the reference's two calls) - the tokenizer is the caller's (transformers' CLIPTokenizer or
        anything with its call interface), the encoder normally emote_hack_amd.clip_text.CLIPTextModel."""
        batch_size = len(prompt) if isinstance(prompt, list) else 1
        tok, enc = self.tokenizer, self.text_encoder
        text_inputs = tok(prompt, padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt")
        text_input_ids = text_inputs.input_ids
        untruncated_ids = tok(prompt, padding="longest", return_tensors="pt").input_ids
        if untruncated_ids.shape[-1] >= text_input_ids.shape[-1] and not torch.equal(text_input_ids, untruncated_ids):
            removed_text = tok.batch_decode(untruncated_ids[:, tok.model_max_length - 1:-1])
            logger.warning("The following part of your input was truncated because CLIP can only handle sequences up to"
                           f" {tok.model_max_length} tokens: {removed_text}")
        use_mask = bool(getattr(getattr(enc, "config", None), "use_attention_mask", False))
        ids, masks = [text_input_ids], [text_inputs.attention_mask] if use_mask else None
        if do_classifier_free_guidance:
            if negative_prompt is None:
                uncond_tokens = [""] * batch_size
            elif type(prompt) is not type(negative_prompt):
                raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} !="
                                f" {type(prompt)}.")
            elif isinstance(negative_prompt, str):
                uncond_tokens = [negative_prompt]
            elif batch_size != len(negative_prompt):
                raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`:"
                                 f" {prompt} has batch size {batch_size}. Please make sure that passed `negative_prompt` matches"
                                 " the batch size of `prompt`.")
            else:
                uncond_tokens = negative_prompt
            uncond_input = tok(uncond_tokens, padding="max_length", max_length=text_input_ids.shape[-1], truncation=True, return_tensors="pt")
            ids.insert(0, uncond_input.input_ids)
            if use_mask:
                masks.insert(0, uncond_input.attention_mask)
        emb = enc(torch.cat(ids).to(device), attention_mask=torch.cat(masks).to(device) if use_mask else None)[0]
        # duplicate the embeddings for each generation per prompt (:231-234, :276-279), uncond half first
        halves = emb.split(batch_size) if do_classifier_free_guidance else (emb,)
        halves = [e.repeat(1, num_videos_per_prompt, 1).view(e.shape[0] * num_videos_per_prompt, e.shape[1], -1) for e in halves]
        return torch.cat(halves) if do_classifier_free_guidance else halves[0]

    @torch.no_grad()
    def _encode_image(self, image, device, num_videos_per_prompt, do_classifier_free_guidance):
        """The image counterpart of _encode_prompt: the cross-attention context from `image_encoder` (:909-917), ONE token per image.
        Nothing in the reference defines the pairing; this is the convention of the image-variation pipeline whose ctor call those lines
        copy: cond = image_embeds.unsqueeze(1), uncond = zeros of the same shape, order [uncond, cond] as with text.
        image: anything the image processor takes (a PIL image, an (H, W, 3) uint8 array / tensor), or pixel_values (1, 3, S, S) already.
        -> (2, 1, D) = [uncond, cond] under classifier-free guidance, (1, 1, D) without."""
        enc = self.image_encoder
        S = enc.config.image_size
        if torch.is_tensor(image) and image.is_floating_point() and image.dim() == 4 and tuple(image.shape[1:]) == (3, S, S):
            pixel_values = image
        else:
            pixel_values = self.image_processor(image, return_tensors="pt").pixel_values
        cond = enc(pixel_values.to(device)).image_embeds.unsqueeze(1)                          # (b, 1, D)
        cond = cond.repeat(1, num_videos_per_prompt, 1).view(cond.shape[0] * num_videos_per_prompt, 1, -1)
        return torch.cat([torch.zeros_like(cond), cond]) if do_classifier_free_guidance else cond

    @torch.no_grad()
    def images2latents(self, images, dtype=None):
        """EMOAnimationPipeline.py:402-414: uint8 RGB frames (f, h, w, c) -> `/ 127.5 - 1`, 'f h w c -> f c h w',
        `vae.encode(frame)['latent_dist'].mean * 0.18215`, frame by frame."""
        if self.vae is None:
            raise ValueError("images2latents needs a VAE (emote_hack_amd.vae.AutoencoderKL)")
        import numpy as np
        x = torch.from_numpy(np.ascontiguousarray(images)) if isinstance(images, np.ndarray) else torch.as_tensor(images)
        if x.dim() != 4 or x.shape[-1] != 3:
            raise ValueError(f"images2latents: expected (f, h, w, 3) RGB frames, got {tuple(x.shape)}")
        return self._normalised2latents((x.float() / 127.5 - 1.0).permute(0, 3, 1, 2).contiguous())

    def _normalised2latents(self, x):
        return torch.cat([self.vae.encode(x[i:i + 1])["latent_dist"].mean * 0.18215 for i in range(x.shape[0])])

    @staticmethod
    def _device_u8_scaled(frames_u8, divisor, shift=0.0):
        """`x.float() / divisor - shift` of uint8 frames that live on the device, with the HOST's rounding: the 256 possible results are
        computed on the host and gathered (a division by a scalar is a multiplication by its reciprocal on the device, which differs
        in the last bit for some x) - frames decoded on the device give the values the same frames give when passed as a host array"""
        table = torch.arange(256, dtype=torch.float32) / divisor
        if shift:
            table = table - shift
        return table.to(frames_u8.device)[frames_u8.long()]

    @staticmethod
    def _clip_frames(path, n_frames, width, height, who, resample=None, progressive=False):
        """the first n_frames frames of a Motion-JPEG `.avi` file - or of an `.apng` file, an animated `.png`, a numbered `.png` pattern
        such as `pose/%04d.png` or a `.gif` file - as uint8 (n_frames, height, width, 3) on the device (video_io.read_video).
        The reference resizes what it reads through PIL (animation.py:174-185): with resample= (a filter of video_io.RESIZE_FILTERS; PIL's
        own default is "bicubic") frames of another size are resized on the device as PIL would (video_io.resize_frames); with None
        another size is refused.  progressive=True takes progressive frames in the clip too (video_io.decode_mjpeg)."""
        from . import video_io
        # existing host tests replace video_io.read_video by a stand-in without the keyword: it is handed over only when set
        frames, _, _ = video_io.read_video(path, length=n_frames, **(dict(progressive=True) if progressive else {}))
        if frames.shape[0] < n_frames:
            raise ValueError(f"{who}={os.fspath(path)!r} holds {frames.shape[0]} frames, {n_frames} are needed: pass a clip at least as long as "
                             "video_length")
        if tuple(frames.shape[1:3]) != (height, width):
            if resample is None:
                raise ValueError(f"{who}={os.fspath(path)!r} holds frames of {frames.shape[1]} x {frames.shape[2]} (height x width), the call runs at "
                                 f"{height} x {width}: frames are not resized here, pass frames at size (or input_resample=\"bicubic\" to have "
                                 "them resized on the device as PIL does)")
            frames = video_io.resize_frames(frames, (width, height), resample)
        return frames

    def _source_image_latents(self, source_image, width, height, resample=None, progressive=False):
        """:686-689: a path is opened and resized to (width, height); an (H, W, 3) uint8 array is taken as it is.  A Motion-JPEG `.avi`
        path gives its first frame (animation.py:182-185), decoded on the device at (height, width) - resized there under resample=, as
        _clip_frames does - and encoded from there.  A baseline `.jpg` / `.jpeg` path is decoded and resized to (width, height) on the
        device as well (video_io.read_image, byte for byte the pixels PIL's open + resize give); what parse_jpeg refuses is PIL's - a
        progressive file too, unless progressive=True sends a complete progression down the same device path.  A `.png` path is PIL's
        too; video_io.read_image decodes one on the device for a caller that wants the pixels there.  So is a `.gif` path: PIL opens its
        first frame, and video_io.read_image gives the same pixels on the device."""
        rgb = self._source_image_rgb(source_image, width, height, resample, progressive)
        if torch.is_tensor(rgb):          # a still JPEG or the first frame of a clip, on the device
            if self.vae is None:
                raise ValueError("images2latents needs a VAE (emote_hack_amd.vae.AutoencoderKL)")
            return self._normalised2latents(self._device_u8_scaled(rgb[None], 127.5, 1.0).permute(0, 3, 1, 2).contiguous())
        return self.images2latents(rgb[None], None)

    @staticmethod
    def _source_image_rgb(source_image, width, height, resample=None, progressive=False):
        import numpy as np
        if isinstance(source_image, (str, os.PathLike)) and os.fspath(source_image).lower().endswith(".avi"):
            # animation.py:182-185 takes the source image from a video's first frame: decoded on the device, and it stays there
            frame = EMOAnimationPipeline._clip_frames(source_image, 1, width, height, "source_image", resample, progressive)[0]
            if frame.shape[0] % 8 or frame.shape[1] % 8:
                raise ValueError(f"source_image {tuple(frame.shape[:2])} must be a multiple of 8 in both directions")
            return frame
        if isinstance(source_image, str) and source_image.lower().endswith((".jpg", ".jpeg")):
            # a baseline JPEG file is decoded and resized on the device (read_image: both byte for byte as Pillow does, "bicubic" being
            # the filter of the `.resize((width, height))` below) and stays there; what parse_jpeg refuses - a progressive file without
            # progressive=True, an incomplete progression with it - is Pillow's, like every other format
            from . import video_io
            with open(source_image, "rb") as f:
                data = f.read()
            try:
                video_io.parse_jpeg(data, restart=True, layouts=True, progressive=progressive)
            except ValueError:
                data = None
            if data is not None:
                frame = video_io.read_image(data, size=(width, height), resample="bicubic", progressive=progressive)
                if frame.shape[0] % 8 or frame.shape[1] % 8:
                    raise ValueError(f"source_image {tuple(frame.shape[:2])} must be a multiple of 8 in both directions")
                return frame
        if isinstance(source_image, str):
            from PIL import Image
            source_image = np.array(Image.open(source_image).convert("RGB").resize((width, height)))
        elif torch.is_tensor(source_image):
            source_image = source_image.detach().cpu().numpy()
        if not isinstance(source_image, np.ndarray) or source_image.ndim != 3 or source_image.shape[-1] != 3:
            raise ValueError("source_image must be a file path or an (H, W, 3) uint8 RGB array (EMOAnimationPipeline.py:686-689)")
        if source_image.shape[0] % 8 or source_image.shape[1] % 8:
            raise ValueError(f"source_image {source_image.shape[:2]} must be a multiple of 8 in both directions")
        return source_image

    # ------------------------------------------------------------------ the rest of the reference class's surface
    def prepare_latents(self, batch_size, num_channels_latents, video_length, height, width, dtype, device, generator, latents=None, clip_length=16):
        """EMOAnimationPipeline.py:341-368: noise for `clip_length` frames, TILED video_length // clip_length times along the frame axis (so a
        video_length < 16 yields an empty tensor upstream - pass `latents` / `init_latents` there), times `scheduler.init_noise_sigma`.  Host
        RNG, like the reference (`torch.randn(shape, generator=generator)`)."""
        shape = (batch_size, num_channels_latents, clip_length, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                             f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        device = torch.device(device)
        if latents is None:
            if isinstance(generator, list):
                latents = torch.cat([torch.randn(shape, generator=generator[i], device=generator[i].device, dtype=dtype) for i in range(batch_size)], dim=0).to(device)
            else:
                latents = torch.randn(shape, generator=generator, device=generator.device if generator is not None else device, dtype=dtype).to(device)
            latents = latents.repeat(1, 1, video_length // clip_length, 1, 1)
        else:
            if tuple(latents.shape) != shape:
                raise ValueError(f"Unexpected latents shape, got {latents.shape}, expected {shape}")
            latents = latents.to(device)
        return latents * self.scheduler.init_noise_sigma

    def prepare_condition(self, condition, num_videos_per_prompt, device, dtype, do_classifier_free_guidance):
        """:370-377: uint8 (f, h, w, c) conditioning frames -> / 255, one copy per video, 'b f h w c -> (b f) c h w', doubled under CFG."""
        import numpy as np
        condition = torch.from_numpy(np.ascontiguousarray(condition).copy()).to(device=device, dtype=dtype) / 255.0
        condition = torch.stack([condition for _ in range(num_videos_per_prompt)], dim=0)
        condition = condition.permute(0, 1, 4, 2, 3).reshape(-1, condition.shape[4], condition.shape[2], condition.shape[3]).clone()
        return torch.cat([condition] * 2) if do_classifier_free_guidance else condition

    def select_controlnet_res_samples(self, controlnet_res_samples_cache_dict, context, do_classifier_free_guidance, b, f):
        """:514-540: the cached per-frame ControlNet residuals of the windows in `context`, '(b f) c h w -> b c f h w', repeated for CFG
        (the loop itself keeps this cache in rows - `_controlnet_residuals`; this is the reference's tensor-level helper)."""
        frames = [i for c in context for i in c]
        n_down = len(controlnet_res_samples_cache_dict[frames[-1]][0])
        down = [torch.cat([controlnet_res_samples_cache_dict[i][0][k] for i in frames]) for k in range(n_down)]
        mid = torch.cat([controlnet_res_samples_cache_dict[i][1] for i in frames])
        b = b // 2 if do_classifier_free_guidance else b

        def to5(t):
            t = t.reshape(b, f, *t.shape[1:]).permute(0, 2, 1, 3, 4)
            return t.repeat(2, 1, 1, 1, 1) if do_classifier_free_guidance else t
        return [to5(t) for t in down], to5(mid)

    @torch.no_grad()
    def decode_latents(self, latents, rank=0, decoder_consistency=None):
        """:291-307: latents / 0.18215 -> the VAE decoder frame by frame (or `decoder_consistency(frame_latents)`) -> (b, 3, f, H, W) in
        [0, 1] as a float32 numpy array."""
        if decoder_consistency is not None:
            f = latents.shape[2]
            lat = (1 / 0.18215 * latents).permute(0, 2, 1, 3, 4).reshape(-1, *latents.shape[1:2], *latents.shape[3:])
            video = torch.cat([decoder_consistency(lat[i:i + 1]) for i in range(lat.shape[0])])
            video = video.reshape(-1, f, *video.shape[1:]).permute(0, 2, 1, 3, 4)
            return (video / 2 + 0.5).clamp(0, 1).cpu().float().numpy()
        if self.vae is None:
            raise ValueError("decode_latents needs a VAE (emote_hack_amd.vae.AutoencoderKL)")
        return self.vae.decode_video(latents).cpu().float().numpy()

    def next_step(self, model_output, timestep: int, x, eta=0., verbose=False):
        """:379-400 - one step of DDIM INVERSION (x_t -> x_{t + T/n}): pred_x0 = (x - sqrt(1 - a) eps) / sqrt(a) with a taken one stride BELOW
        `timestep` (final_alpha_cumprod below 0), x_next = sqrt(a_next) pred_x0 + sqrt(1 - a_next) eps.  Returns (x_next, pred_x0).  Scalars
        on the host in f64; the two linear combinations run as emo_add launches on the device (plain torch for CPU tensors)."""
        sch = self.scheduler
        if verbose:
            print("timestep: ", timestep)
        nxt = int(timestep)
        t = min(nxt - sch.config.num_train_timesteps // sch.num_inference_steps, 999)
        a_t = float(sch.alphas_cumprod[t]) if t >= 0 else float(sch.final_alpha_cumprod)
        a_next = float(sch.alphas_cumprod[nxt])
        k0x, k0e = 1.0 / a_t ** 0.5, -((1.0 - a_t) ** 0.5) / a_t ** 0.5               # pred_x0 = k0x x + k0e eps
        knx, kne = a_next ** 0.5 * k0x, a_next ** 0.5 * k0e + (1.0 - a_next) ** 0.5    # x_next  = knx x + kne eps

        def lincomb(cx, ce):
            if not x.is_cuda:
                return cx * x + ce * model_output
            xf, ef = x.float().reshape(1, -1).contiguous(), model_output.float().reshape(1, -1).contiguous()
            z = ops.add(xf, ef, alpha=ce / cx)                     # x + (ce / cx) eps
            return ops.add(z, z, alpha=cx - 1.0).reshape(x.shape).to(x.dtype)      # ... times cx
        return lincomb(knx, kne), lincomb(k0x, k0e)

    @torch.no_grad()
    def invert(self, image, prompt=None, num_inference_steps=20, num_actual_inference_steps=10, eta=0.0, return_intermediates=False, **kwargs):
        """:417-477 - deterministic DDIM inversion of real frames into a noise map: frames -> latents (`images2latents`, or pass
        latents=(f, 4, h, w)), then for the ascending timesteps x <- next_step(unet(x as one (1, c, f, h, w) clip, t, text), t, x), stopping after
        `num_actual_inference_steps`.  The prompt goes through the tokenizer + text encoder on the pipeline, called like upstream
        (emote_hack_amd.clip_text.CLIPTextModel runs it on these kernels); or pass text_embeddings=(1, L, D)."""
        text_embeddings = kwargs.get("text_embeddings")
        if text_embeddings is None:
            if self.text_encoder is None or self.tokenizer is None:
                raise ValueError("invert: pass text_embeddings=(1, L, D), or put a tokenizer + text_encoder on the pipeline")
            text_input = self.tokenizer(prompt, padding="max_length", max_length=self.tokenizer.model_max_length, return_tensors="pt")
            text_embeddings = self.text_encoder(text_input.input_ids.to(self._execution_device))[0]
        latents = kwargs.get("latents")
        if latents is None:
            latents = self.images2latents(image)
        latents = latents.to(self._execution_device)
        self.scheduler.set_timesteps(num_inference_steps)
        latents_list, pred_x0_list = [latents], [latents]
        for i, t in enumerate(reversed(self.scheduler.timesteps)):
            if num_actual_inference_steps is not None and i >= num_actual_inference_steps:
                continue
            model_inputs = latents.permute(1, 0, 2, 3).unsqueeze(0)                          # 'f c h w -> 1 c f h w'
            noise_pred = self.unet(model_inputs, int(t), encoder_hidden_states=text_embeddings).sample
            noise_pred = noise_pred[0].permute(1, 0, 2, 3)                                   # 'b c f h w -> (b f) c h w'
            latents, pred_x0 = self.next_step(noise_pred.to(latents.dtype), int(t), latents)
            latents_list.append(latents)
            pred_x0_list.append(pred_x0)
        if return_intermediates:
            return latents, latents_list
        return latents

    def interpolate_latents(self, latents: torch.Tensor, interpolation_factor: int, device):
        """:479-512: `interpolation_factor - 1` frames interpolated between every two consecutive frames with the method set by
        `set_tensor_interpolation_method` (magicanimate/utils/util.py:116-140: slerp over the whole frame tensor, linear when the two are
        nearly parallel).  The reference's `__call__` hard-codes the factor 1 (:824), for which this is the identity; ours takes
        `interpolation_factor=`.  Latents on a HIP device with this module's own `slerp` / `linear` set go through emo_interp_frames (two
        launches for the clip, the threshold branch on the device); CPU tensors and a user-installed callable take the host-level torch
        path below."""
        if interpolation_factor < 2:
            return latents
        method = get_tensor_interpolation_method()
        if method is None:
            raise TypeError("'NoneType' object is not callable: call set_tensor_interpolation_method(is_slerp) first (magicanimate/utils/util.py:116-123)")
        return self._interpolate_latents(latents, interpolation_factor, device, method)

    def _interpolate_latents(self, latents, interpolation_factor, device, method):
        if latents.is_cuda and (method is slerp or method is linear):
            x = latents if latents.dtype == torch.float32 else ops.convert(latents, torch.float32)
            y = ops.interpolate_frames(x, interpolation_factor, "slerp" if method is slerp else "linear")
            return y if latents.dtype == torch.float32 else ops.convert(y, latents.dtype)
        n = latents.shape[2]
        out = torch.zeros((latents.shape[0], latents.shape[1], (n - 1) * interpolation_factor + 1, latents.shape[3], latents.shape[4]),
                          device=latents.device, dtype=latents.dtype)
        rate = [i / interpolation_factor for i in range(interpolation_factor)][1:]
        k = 0
        for i0 in range(n - 1):
            v0, v1 = latents[:, :, i0], latents[:, :, i0 + 1]
            out[:, :, k] = v0
            k += 1
            for fr in rate:
                out[:, :, k] = method(v0.to(device=device), v1.to(device=device), fr).to(latents.device)
                k += 1
        out[:, :, k] = latents[:, :, n - 1]
        return out

    @staticmethod
    def _audio_for_file(audio):
        """the samples save_path= puts beside the frames: audio= as a `.wav` path or a (samples, rate) pair, at its own rate and with its
        own channels -> (float samples (n, channels), rate); anything else (a bare waveform, a container this build cannot demux) -> None"""
        if isinstance(audio, (str, os.PathLike)):
            if not os.fspath(audio).lower().endswith(".wav"):
                return None
            from .audio_io import read_wav
            return read_wav(audio)
        if isinstance(audio, tuple) and len(audio) == 2 and isinstance(audio[1], numbers.Integral):
            x = audio[0].detach().cpu() if torch.is_tensor(audio[0]) else torch.as_tensor(audio[0])
            return (x.reshape(len(x), -1).float().numpy(), int(audio[1]))
        return None

    def _encode_head_speeds(self, speeds, video_length=None):
        """head speeds through the pipeline's SpeedEncoder: ONE per clip (head_rotation_speeds=) -> (1, 4*C0), or with video_length one per
        frame (head_speeds_per_frame=) -> (1, video_length, 4*C0)"""
        keyword, shape = ("head_rotation_speeds", "1, ") if video_length is None else ("head_speeds_per_frame", "1, video_length, ")
        enc = getattr(self, "speed_encoder", None)
        if enc is None:
            raise ValueError(f"{keyword}= needs a speed_encoder on the pipeline (emote_hack_amd.conditioning.SpeedEncoder(9, "
                             "4 * block_out_channels[0]) with loaded weights: pass speed_encoder= to the constructor or assign "
                             f"pipe.speed_encoder), or pass speed_embeddings=({shape}4 * block_out_channels[0])")
        v = torch.as_tensor(speeds, dtype=torch.float32).reshape(-1)
        if video_length is not None and v.numel() != video_length:
            raise ValueError(f"head_speeds_per_frame= takes one speed per frame: got {v.numel()} values for video_length {video_length}")
        if video_length is None and v.numel() != 1:
            raise ValueError(f"head_rotation_speeds= takes ONE speed per clip (a float or a one-element tensor), got {v.numel()} values: "
                             "per-frame speeds would need a per-frame time embedding - run one clip per speed, or pass speed_embeddings=")
        width_e = 4 * self.unet.config.block_out_channels[0]      # (the UNet's time-embedding width)
        if enc.speed_embedding_dim != width_e:
            raise ValueError(f"the speed_encoder embeds to {enc.speed_embedding_dim} values, the UNet's time embedding has {width_e}: "
                             f"build SpeedEncoder(9, {width_e})")
        return enc(v) if video_length is None else enc(v).reshape(1, video_length, width_e)

    # ------------------------------------------------------------------ reference-compatible entry point
    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str]], video_length: Optional[int], height: Optional[int] = None,
                 width: Optional[int] = None, num_inference_steps: int = 50, guidance_scale: float = 7.5,
                 negative_prompt=None, num_videos_per_prompt: Optional[int] = 1, eta: float = 0.0, generator=None,
                 latents=None, output_type: Optional[str] = "tensor", return_dict: bool = True,
                 callback: Optional[Callable] = None, callback_steps: Optional[int] = 1, controlnet_condition: list = None,
                 controlnet_conditioning_scale: float = 1.0, context_frames: int = 16, context_stride: int = 1,
                 context_overlap: int = 4, context_batch_size: int = 1, context_schedule: str = "uniform",
                 init_latents=None, num_actual_inference_steps: Optional[int] = None, appearance_encoder=None,
                 reference_control_writer=None, reference_control_reader=None, source_image=None,
                 decoder_consistency=None, audio=None, head_rotation_speeds=None, **kwargs):
        """Signature = EMOAnimationPipeline.py:544-578.  `prompt` / `negative_prompt` are encoded by `_encode_prompt` when the
        pipeline has a tokenizer (and a text encoder, e.g. emote_hack_amd.clip_text.CLIPTextModel); text_embeddings=(2,L,D) takes precedence.
        clip_image= (with prompt "") conditions on an image instead: `_encode_image` runs the pipeline's image_encoder on it.
        audio= is a .wav path (any sample rate, any channel count: read, downmixed, resampled to 16 kHz and normalised by
        emote_hack_amd.audio_io, then wav2vec2 through feature_extractor=), a (samples, sample_rate) pair, or a bare waveform at 16 kHz
        (audio_sample_rate= names another rate).  fps= (an int, a Fraction or a (num, den) pair) with audio_start= seconds keeps time:
        video frame i takes the wav2vec2 frame at audio_start + i / fps (ValueError when the audio ends before the clip); without fps
        the audio is stretched over the clip.  head_rotation_speeds= is ONE speed per clip (a float or a one-element f32 tensor) encoded by
        the pipeline's speed_encoder into `speed_embeddings` (one shared row); the reference's own `SpeedEncoder(10, 64)` asserts at
        Net.py:212 (9 bucket centres), so 9 buckets is the constructible choice, at the UNet's time-embedding width.
        head_speeds_per_frame= is `video_length` speeds, one per frame, encoded once into a (video_length, 4*C0) table of per-frame speed
        embeddings (the time embedding then differs per frame; not together with head_rotation_speeds=).  face_mask= is the face region: an
        (H, W) or (1, 1, H, W) bool / uint8 / float map at (height, width) - pooled 8 x 8 - or at latent size, or "locate" = the pipeline's
        face_locator run on source_image (logit > 0); the pipeline's face_region_controller turns it into features added behind conv_in for
        every frame and both guidance branches (face_mask_threshold=t pools mask > t instead of the mask).
        Extra keyword inputs for the parts that are out of scope here: ref_image_latents=(1,4,h,w), audio_features=(F,L_a,D),
        speed_embeddings=(1 | 2, 4*C0) per clip or (1 | 2, video_length, 4*C0) per frame, shared or [uncond, cond] (takes precedence over
        head_rotation_speeds / head_speeds_per_frame), seed=int; dist/rank/world_size as in the reference (:636-638).  Execution knobs (all
        optional): use_graphs (default: HIP-graph replay on a HIP device - the path bench.py measures), reference_group
        (ReferenceNet timesteps per batched pass; default 10, the configuration bench.py measures - 25 would make two passes per 50-step clip,
        40.03 vs 40.38 ms per step), reference_lookahead, fusion_blocks, motion_latents, reuse_state
        (default True: a second call with the same geometry reuses the prepared plan and its captured graphs).
        interpolation_factor=k (an int >= 1, default 1 as :824 hard-codes) puts k - 1 interpolated frames between every two denoised
        frames, where upstream has the stage: after the loop, before the decode (`interpolate_latents`, one emo_interp_frames call on the
        finished latents; every rank of a dist=True run interpolates its identical copy).  interpolation="slerp" | "linear" picks the
        method for this call only; None takes the one set by `set_tensor_interpolation_method`, slerp when none was set.
        output_type="uint8" returns `videos` as (1, frames, H, W, 3) uint8 on the device (AutoencoderKL.decode_video(output="uint8"));
        "latent" returns the (interpolated) latents.
        save_path="clip.avi" (with save_quality=1 .. 100, default 90) also writes the clip, where every reference run ends in
        `save_videos_grid` (magicanimate/utils/util.py:21-33): the latents are decoded as for output_type="uint8" (so a VAE is needed),
        JPEG-encoded on the device and written as Motion-JPEG in an AVI container (emote_hack_amd.video_io) playing at fps *
        interpolation_factor - fps= is required.  audio= given as a `.wav` path or a (samples, rate) pair goes into the file as 16-bit PCM,
        with its own channels at its own rate, from audio_start for the clip's duration (less where the audio ends first).  The return
        value is what it is without save_path.  save_restart_interval="row" (one row of MCUs) or a number of MCUs from 1 to 65535 cuts
        every frame's scan into restart intervals (a DRI segment and RSTm markers, T.81 E.1.4), which video_io.decode_mjpeg decodes in
        parallel; None, the default, writes the files written without it.
        save_path="clip.gif" writes an animated GIF instead, the other file `imageio.mimsave` is asked for: the same 8-bit frames are
        quantised to 256 colours, mapped and LZW-coded on the device (emote_hack_amd.video_io.encode_gif) and play at fps *
        interpolation_factor, which may not pass 50.  save_palette="global" | "frame" (one colour table for the clip, the default, or one
        per frame), save_dither=None | "bayer" with save_dither_strength=1 .. 128 (default 32) and save_loop=0 .. 65535 (0, the
        default: forever) are its options.  A GIF has no sound: audio= still drives the model and is not in the file.  A save_* keyword
        that belongs to another format than save_path's is refused by the name of that format, whichever the formats
        (emote_hack_amd.video_io.save_plan checks the call against the one table of formats, video_io.FORMATS, before anything runs).
        save_path="clip.apng" writes a lossless animated PNG of the same 8-bit frames, filtered, matched and Huffman-coded on the device
        (emote_hack_amd.video_io.encode_apng), playing at exactly fps * interpolation_factor (the reduced fraction's terms must fit 16
        bits); save_path="frames/f_%04d.png" - a `.png` name with one %d-style field - writes every frame as a numbered PNG still,
        counted from 0, and needs no fps= (a plain `.png` name takes a one-frame clip).  save_png_filter="adaptive" (the default) |
        "none" | "sub" | "up" | "average" | "paeth" is their option, save_loop= the `.apng`'s; the JPEG and GIF options are refused
        with them, and audio= is not in the files.
        input_resample="bicubic" | "box" | "bilinear" | "hamming" | "lanczos" lets clips come at any size: a controlnet_condition= clip
        path or a source_image= `.avi` path whose frames are not height x width is resized on the device, byte for byte as the
        `Image.resize` of animation.py:174-185 would ("bicubic" is that call's filter; emote_hack_amd.video_io.resize_frames).  None, the
        default, refuses such a clip as before.  Host arrays and image files are not touched by it, and a clip shorter than
        video_length is refused either way.
        input_progressive=True decodes progressive JPEGs (SOF2, a complete progression) on the device too: a source_image= `.jpg` /
        `.jpeg` path, which otherwise goes through PIL on the host, and progressive frames inside a controlnet_condition= or
        source_image= clip, which are otherwise refused (emote_hack_amd.video_io.decode_mjpeg(progressive=True); the pixels are
        PIL's byte for byte).  False, the default, launches what it launched before."""
        input_progressive = kwargs.get("input_progressive", False)
        if not isinstance(input_progressive, bool):
            raise ValueError(f"input_progressive= takes True or False, got {input_progressive!r}")
        input_resample = kwargs.get("input_resample")
        if input_resample is not None:
            from . import video_io
            input_resample = video_io._resize_filter(input_resample)
        interp_k, interp = kwargs.get("interpolation_factor", 1), kwargs.get("interpolation")
        if isinstance(interp_k, bool) or not isinstance(interp_k, numbers.Integral) or interp_k < 1:
            raise ValueError(f"interpolation_factor= takes an int >= 1 (1: no interpolated frames), got {interp_k!r}")
        if interp is not None and interp not in ("slerp", "linear"):
            raise ValueError(f"interpolation= takes None (the method set by set_tensor_interpolation_method), \"slerp\" or \"linear\", got {interp!r}")
        if interp_k >= 2 and (video_length is None or video_length < 2):
            raise ValueError(f"interpolation_factor={interp_k} interpolates between consecutive frames: video_length must be >= 2, got {video_length!r}")
        if output_type == "uint8" and self.vae is None:
            raise ValueError("output_type=\"uint8\" decodes the latents into 8-bit frames: it needs a VAE on the pipeline "
                             "(emote_hack_amd.vae.AutoencoderKL, vae= of the constructor); output_type=\"latent\" returns the latents")
        plan = save_audio = None
        if kwargs.get("save_path") is not None:      # what the path and the save_* keywords can be refused for, before anything runs
            from . import video_io
            from .conditioning import _as_fraction
            plan = video_io.save_plan(kwargs["save_path"], (int(video_length) - 1) * int(interp_k) + 1 if video_length else 1,
                                      None if kwargs.get("fps") is None else _as_fraction(kwargs["fps"], "fps"), interp_k,
                                      {name: kwargs.get(keyword) for name, keyword in video_io.SAVE_KEYWORDS.items()})
            if plan.record.plays and plan.rate is None:
                raise ValueError("save_path= writes a video file and a file has a frame rate: pass fps= (an int, a Fraction or a (num, den) "
                                 "pair; the file plays at fps * interpolation_factor)")
            if self.vae is None:
                raise ValueError("save_path= decodes the latents into 8-bit frames, as output_type=\"uint8\" does: it needs a VAE on the pipeline "
                                 "(emote_hack_amd.vae.AutoencoderKL, vae= of the constructor)")
            if plan.record.sound:
                save_audio = self._audio_for_file(audio)
        height = height or self.unet.config.sample_size * self.vae_scale_factor
        width = width or self.unet.config.sample_size * self.vae_scale_factor
        self.check_inputs(prompt, height, width, callback_steps)
        assert num_videos_per_prompt == 1   # :641
        if isinstance(prompt, list) and len(prompt) != 1:
            raise AssertionError("batch_size == 1")  # :642
        cn_cond = None
        if self.controlnet is not None:
            if controlnet_condition is None:
                raise ValueError("controlnet_condition (F,H,W,3 uint8 frames or a (F,3,H,W) float tensor) is required with a ControlNet")
            # prepare_condition (:369-376): uint8 HWC frames / 255 -> (f, c, h, w)
            from_clip = isinstance(controlnet_condition, (str, os.PathLike))
            if from_clip:
                # animation.py:174-180 reads the control sequence from a video file: the first video_length frames, decoded on the device
                controlnet_condition = self._clip_frames(controlnet_condition, video_length, width, height, "controlnet_condition", input_resample,
                                                          input_progressive)
            cn_cond = controlnet_condition if torch.is_tensor(controlnet_condition) else torch.as_tensor(controlnet_condition)
            if from_clip:
                cn_cond = self._device_u8_scaled(cn_cond, 255.0).permute(0, 3, 1, 2)
            if cn_cond.dim() == 4 and cn_cond.shape[-1] == 3 and cn_cond.shape[1] != 3:
                cn_cond = cn_cond.permute(0, 3, 1, 2).float() / 255.0
            cn_cond = cn_cond.float()
        elif controlnet_condition is not None:
            raise ValueError("controlnet_condition given but the pipeline has no controlnet")
        if appearance_encoder is None:
            raise ValueError("appearance_encoder (ReferenceNet) is required")
        text_embeddings = kwargs.get("text_embeddings")
        clip_image = kwargs.get("clip_image")
        if clip_image is not None:      # image conditioning: the context is the image encoder's one token (_encode_image)
            if getattr(self, "image_encoder", None) is None:
                raise ValueError("clip_image= needs an image_encoder on the pipeline (emote_hack_amd.clip_vision.CLIPVisionModelWithProjection)")
            if text_embeddings is not None:
                raise ValueError("clip_image= and text_embeddings= both name the cross-attention context: pass one")
            if prompt not in ("", [""]):
                raise ValueError("clip_image= replaces the prompt as the cross-attention context: call with prompt \"\"")
            text_embeddings = self._encode_image(clip_image, self._execution_device, num_videos_per_prompt, self._do_cfg(guidance_scale))
        if text_embeddings is None:
            if self.text_encoder is None:
                raise ValueError("pass text_embeddings=(2,L,D) [uncond, cond], or put a tokenizer + text_encoder "
                                 "(emote_hack_amd.clip_text.CLIPTextModel) on the pipeline")
            if self.tokenizer is not None:     # :628-630
                text_embeddings = self._encode_prompt(prompt, self._execution_device, num_videos_per_prompt, self._do_cfg(guidance_scale),
                                                      negative_prompt)
            else:
                text_embeddings = self.text_encoder(prompt, negative_prompt)
        ref_lat = kwargs.get("ref_image_latents")
        if ref_lat is None:
            if self.vae is None or source_image is None:
                raise ValueError("pass ref_image_latents=(1,4,h,w) (no VAE in this build)")
            ref_lat = self._source_image_latents(source_image, width, height, input_resample, input_progressive)   # :686-689 -> images2latents (:402-414)
        if audio is not None and kwargs.get("audio_features") is None:
            # :592-593 `audio_features = feature_extractor.extract_features_from_mp4(audio, m=2, n=2)` (a module-level extractor
            # there; the file read, resampling and channel mean of Net.py:627-640 behind it): feature_extractor= is an
            # emote_hack_amd.wav2vec2.Wav2VecFeatureExtractor with caller-loaded weights
            fx = kwargs.get("feature_extractor")
            if fx is None:
                raise ValueError("audio= needs feature_extractor= (emote_hack_amd.wav2vec2.Wav2VecFeatureExtractor), or pass audio_features=")
            from .conditioning import audio_context_tokens
            rate = kwargs.get("audio_sample_rate")
            if isinstance(audio, bytes):
                raise ValueError("audio= takes a .wav path, a (samples, sample_rate) pair or a waveform, not the file's bytes")
            if isinstance(audio, (str, os.PathLike)):
                if rate is not None:
                    raise ValueError("audio_sample_rate= names the rate of a bare waveform; a file carries its own")
                path = os.fspath(audio)
                windows = (fx.extract_features_from_wav if path.lower().endswith(".wav") else fx.extract_features_from_mp4)(path, m=2, n=2)
            else:
                if isinstance(audio, tuple) and len(audio) == 2 and isinstance(audio[1], numbers.Integral):
                    if rate is not None and int(rate) != audio[1]:
                        raise ValueError(f"audio=(samples, {audio[1]}) and audio_sample_rate={rate} disagree")
                    audio, rate = audio[0], int(audio[1])
                # a bare waveform without a rate stays "mono or multi-channel at 16 kHz", on the host path as before
                windows = fx.extract_features(audio, m=2, n=2) if rate is None else fx.extract_features(audio, m=2, n=2, sample_rate=int(rate))
            cfg = fx.model.config
            kwargs["audio_features"] = audio_context_tokens(windows, video_length, cfg.hidden_size, fps=kwargs.get("fps"),
                                                            audio_start=kwargs.get("audio_start", 0),
                                                            audio_frame_rate=(fx.sampling_rate, math.prod(cfg.conv_stride)))
        if kwargs.get("head_speeds_per_frame") is not None:
            # one speed per FRAME: the whole clip goes through the SpeedEncoder once, and the UNet takes the (video_length, 4*C0) table as
            # per-frame speed embeddings (each UNet call gathers its windows' rows)
            if head_rotation_speeds is not None:
                raise ValueError("head_rotation_speeds= (ONE speed per clip) and head_speeds_per_frame= both name the head speed: pass one")
            if kwargs.get("speed_embeddings") is None:
                kwargs["speed_embeddings"] = self._encode_head_speeds(kwargs["head_speeds_per_frame"], video_length)
        if head_rotation_speeds is not None and kwargs.get("speed_embeddings") is None:
            # :783-784 hands `head_rotation_speeds` to a UNet that rejects it; here ONE speed per clip goes through the pipeline's
            # SpeedEncoder (Net.py:198-258) into the UNet's class-embedding slot, one row shared by the CFG halves
            kwargs["speed_embeddings"] = self._encode_head_speeds(head_rotation_speeds)
        self._check_speed_embeddings(kwargs.get("speed_embeddings"), video_length)
        face_mask, face_thr = kwargs.get("face_mask"), kwargs.get("face_mask_threshold")
        if face_mask is not None:
            # EMO's face region (Net.py:509-516): a mask, or "locate" = where the pipeline's FaceLocator (Net.py:819-855) sees a face in the
            # source image (logit > 0, i.e. sigmoid > 0.5); the FaceRegionController turns it into features behind conv_in, once per clip
            if self._check_face_mask(face_mask, height, width, locate_ok=True) == "locate":
                loc = getattr(self, "face_locator", None)
                if loc is None:
                    raise ValueError("face_mask=\"locate\" needs a face_locator on the pipeline (emote_hack_amd.conditioning.FaceLocator with loaded "
                                     "weights: pass face_locator= to the constructor or assign pipe.face_locator), or pass the mask itself")
                if source_image is None:
                    raise ValueError("face_mask=\"locate\" looks for the face in source_image=: pass it (a path or an (H, W, 3) uint8 array), or "
                                     "pass the mask itself")
                rgb = self._source_image_rgb(source_image, width, height, input_resample, input_progressive)
                if torch.is_tensor(rgb):      # the first frame of a clip, on the device
                    face_mask = loc(self._device_u8_scaled(rgb, 255.0).permute(2, 0, 1)[None])[0, 0]
                else:
                    face_mask = loc(torch.as_tensor(rgb).permute(2, 0, 1)[None].float() / 255.0)[0, 0]      # logits (H, W); pixels in [0, 1]
                face_thr = 0.0
        if init_latents is not None:   # (b f) c h w -> b c f h w  (:657-658)
            bf, c4, hh, ww = init_latents.shape
            lat = init_latents.reshape(bf // video_length, video_length, c4, hh, ww).permute(0, 2, 1, 3, 4)
        elif latents is not None:
            lat = latents
        else:
            # prepare_latents draws clip_length=16 frames and tiles them video_length//16 times (:341-360)
            if video_length < 16:
                raise ValueError("video_length < 16 needs init_latents (prepare_latents tiles 16-frame noise, :341-360)")
            g = generator if isinstance(generator, torch.Generator) else None
            base = torch.randn(1, self.unet.in_channels, 16, height // 8, width // 8, generator=g)
            lat = base.repeat(1, 1, video_length // 16, 1, 1) * self.scheduler.init_noise_sigma
        lat = self.denoise(lat, ref_lat, text_embeddings, appearance_encoder=appearance_encoder,
                           num_inference_steps=num_inference_steps, guidance_scale=guidance_scale, eta=eta,
                           context_frames=context_frames, context_stride=context_stride, context_overlap=context_overlap,
                           context_batch_size=context_batch_size, context_schedule=context_schedule,
                           audio_features=kwargs.get("audio_features"), speed_embeddings=kwargs.get("speed_embeddings"),
                           face_mask=face_mask, face_mask_threshold=face_thr,
                           seed=kwargs.get("seed", 0), dist=kwargs.get("dist", False), rank=kwargs.get("rank", 0),
                           world_size=kwargs.get("world_size", 1), num_actual_inference_steps=num_actual_inference_steps,
                           callback=callback, callback_steps=callback_steps, controlnet=self.controlnet, controlnet_cond=cn_cond,
                           controlnet_conditioning_scale=controlnet_conditioning_scale,
                           # the measured path: HIP-graph replay (default on a HIP device), batched ReferenceNet groups, and the
                           # prepared state kept for the next clip of the same geometry
                           use_graphs=kwargs.get("use_graphs"), reference_group=kwargs.get("reference_group", 10),   # = the configuration bench.py measures (25: two passes per 50-step clip, -0.35 ms per step)
                           reference_lookahead=kwargs.get("reference_lookahead"), fusion_blocks=kwargs.get("fusion_blocks", "midup"),
                           motion_latents=kwargs.get("motion_latents"), reuse_state=kwargs.get("reuse_state", True),
                           text_pairing=kwargs.get("text_pairing", "reference"))
        if interp_k >= 2:      # :824, between the loop and the decode
            method = {"slerp": slerp, "linear": linear}.get(interp) or get_tensor_interpolation_method() or slerp
            lat = self._interpolate_latents(lat, int(interp_k), lat.device, method)
        frames_u8 = self.vae.decode_video(lat, output="uint8") if output_type == "uint8" or plan is not None else None
        if plan is not None:      # the end of every reference run: save_videos_grid (magicanimate/utils/util.py:21-33)
            if save_audio is not None:
                samples, rate = save_audio
                first = math.floor(_as_fraction(kwargs.get("audio_start", 0), "audio_start") * rate)
                count = math.floor(frames_u8.shape[0] * frames_u8.shape[1] * rate / plan.rate + Fraction(1, 2))
                save_audio = (samples[first:first + count], rate) if first < len(samples) else None      # cut where the audio ends
            plan.write(frames_u8, save_audio)
        if output_type == "uint8":
            video = frames_u8
        elif self.vae is not None and output_type != "latent":
            video = self.vae.decode_video(lat)   # caller-supplied (:291-307)
        else:
            video = lat
        if not return_dict:
            return video
        return AnimationPipelineOutput(videos=video)
