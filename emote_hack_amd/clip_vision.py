"""The CLIP image encoder of the reference on MI355X: `CLIPVisionModelWithProjection`, loaded at EMOAnimationPipeline.py:867 and handed
to the pipeline as `image_encoder=` (:909-917); videonet_animatediff.py:9 imports `CLIPVisionModel` and `CLIPImageProcessor`.  Its
image_embeds are the cross-attention context of the sd-image-variations UNet a VideoNet starts from (`clip_condition_embeddings`,
models/videonet.py:255: one token, 768 wide).  Third-party, weights from the network, so weights are CALLER-LOADED (`load_state_dict`
takes transformers' key names - `vision_model.pre_layrnorm` in the upstream spelling -, `from_pretrained` reads a local folder).

  processor    CLIPImageProcessor: emo_image_preprocess - shortest-edge antialiased bicubic resize, centre crop, rescale, normalise in
               one launch, f32 throughout (tap tables built on the host, only the crop window is computed)
  embeddings   emo_patch_rows (im2col of the stride-P conv, K = 3 P P padded to 8) -> emo_gemm without bias -> emo_vision_embed (class
               token, position embedding and pre_layrnorm in one read and one write) = hidden_states[0]
  N layers     pre-LN, exactly as clip_text runs them, attention NON-causal over Np + 1 tokens (257 for ViT-L/14; V^T ld 264): LN1
               folded into the q | k projection and into the V^T projection (two launches: 257 rows are not a multiple of 32),
               emo_attention, out_proj + residual, LN2 folded into fc1, emo_act, fc2 + residual
  pooling      pooler_output = post_layernorm(last_hidden_state[:, 0]) (emo_layernorm over a strided rows view); image_embeds =
               pooler_output @ visual_projection.weight^T (emo_gemm); last_hidden_state is the encoder output WITHOUT post_layernorm

Pinned by outputs of transformers' own CLIPVisionModelWithProjection and CLIPImageProcessor (tools/oracle/gen_golden_clip_vision.py ->
tests/golden/clip_vision.safetensors).  Not built: interpolate_pos_encoding, output_attentions, CLIPModel (joint text and image,
its logits).
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from ._lib import EmoHipError
from .clip_layers import ACTS as _ACTS, clip_layer_shapes, load_local_checkpoint, pack_clip_layers, run_clip_layers
from .module import HipModule, round_up
from .synth import synth_state_dict

# the vision tower of openai/clip-vit-large-patch14 (= the image_encoder of lambdalabs/sd-image-variations-diffusers)
VITL14_CONFIG = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, num_channels=3, image_size=224,
                     patch_size=14, projection_dim=768, hidden_act="quick_gelu", layer_norm_eps=1e-5)
OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def clip_vision_param_shapes(cfg=None, projection=True):
    """transformers' CLIPVisionModelWithProjection state-dict keys / shapes (projection=False: CLIPVisionModel's - no visual_projection);
    without the non-persistent `position_ids` buffer."""
    c = dict(VITL14_CONFIG, **(cfg or {}))
    H, I, P = c["hidden_size"], c["intermediate_size"], c["patch_size"]
    n_pos = (c["image_size"] // P) ** 2 + 1
    v = "vision_model"
    d = {f"{v}.embeddings.class_embedding": (H,),
         f"{v}.embeddings.patch_embedding.weight": (H, c["num_channels"], P, P),
         f"{v}.embeddings.position_embedding.weight": (n_pos, H),
         f"{v}.pre_layrnorm.weight": (H,),
         f"{v}.pre_layrnorm.bias": (H,)}
    d.update(clip_layer_shapes(f"{v}.encoder.layers", c["num_hidden_layers"], H, I))
    d[f"{v}.post_layernorm.weight"] = (H,)
    d[f"{v}.post_layernorm.bias"] = (H,)
    if projection:
        d["visual_projection.weight"] = (c["projection_dim"], H)
    return d


def clip_vision_synth_state_dict(cfg=None, prefix="clip_vision.", device="cpu", projection=True):
    """Name-keyed synthetic weights (emote_hack_amd.synth) under transformers' key names."""
    return synth_state_dict(clip_vision_param_shapes(cfg, projection), prefix=prefix, device=device)


class CLIPVisionModelOutput(SimpleNamespace):
    """transformers' BaseModelOutputWithPooling surface (CLIPVisionModel): `[0]` last_hidden_state, `[1]` pooler_output, then
    hidden_states when they were asked for."""

    def __getitem__(self, i):
        t = (self.last_hidden_state, self.pooler_output) + ((self.hidden_states,) if self.hidden_states is not None else ())
        return t[i]


class CLIPVisionModelWithProjectionOutput(SimpleNamespace):
    """transformers' CLIPVisionModelOutput surface (CLIPVisionModelWithProjection): `[0]` image_embeds, `[1]` last_hidden_state, then
    hidden_states when they were asked for; `.pooler_output` rides along (the tensor image_embeds is projected from)."""

    def __getitem__(self, i):
        t = (self.image_embeds, self.last_hidden_state) + ((self.hidden_states,) if self.hidden_states is not None else ())
        return t[i]


class CLIPVisionModel(HipModule):
    """forward(pixel_values (B, 3, S, S), S = image_size) -> namespace(last_hidden_state (B, Np + 1, hidden), pooler_output (B, hidden),
    hidden_states) in the model's dtype."""
    _projection = False
    _name = "CLIPVisionModel"
    # older checkpoints carry the position_ids buffer; transformers ignores it (non-persistent).  visual_projection: a with-projection
    # checkpoint read as the bare tower
    _tolerated = frozenset({"vision_model.embeddings.position_ids", "visual_projection.weight"})

    def __init__(self, config=None, **kwargs):
        cfg = dict(VITL14_CONFIG)
        if config is not None:
            cfg.update(config if isinstance(config, dict) else {k: getattr(config, k) for k in VITL14_CONFIG if hasattr(config, k)})
        cfg.update(kwargs)
        cfg = {k: cfg[k] for k in VITL14_CONFIG}
        if cfg["hidden_act"] not in _ACTS:
            raise NotImplementedError(f"{self._name}: hidden_act {cfg['hidden_act']!r} (quick_gelu | gelu)")
        H, nh = cfg["hidden_size"], cfg["num_attention_heads"]
        if H % nh or (H // nh) % 8 or cfg["intermediate_size"] % 8 or cfg["projection_dim"] % 8:
            raise ValueError(f"{self._name}: the head dim and the widths must be multiples of 8")
        if cfg["num_channels"] != 3 or cfg["image_size"] % cfg["patch_size"]:
            raise ValueError(f"{self._name}: 3 input channels and an image_size that is a multiple of patch_size")
        self.config = SimpleNamespace(**cfg)
        self._cfg = cfg
        super().__init__(clip_vision_param_shapes(cfg, self._projection))

    @classmethod
    def from_pretrained(cls, pretrained_model_path, subfolder="image_encoder", torch_dtype=None, **_ignored):
        """A LOCAL checkpoint folder (`<path>/<subfolder>/config.json` + `model.safetensors` or `pytorch_model.bin`), as
        EMOAnimationPipeline.py:867 names it - nothing is fetched."""
        config, sd = load_local_checkpoint(pretrained_model_path, subfolder)
        config = dict(config.get("vision_config") or {}, **config)      # a joint CLIPConfig nests the tower's settings
        model = cls({k: config[k] for k in VITL14_CONFIG if k in config})
        model.load_state_dict(sd)
        if torch_dtype is not None:
            model.to(dtype=torch_dtype)
        return model

    def _pack_weights(self):
        c, dev, dtp, sd = self._cfg, self.device, self.dtype, self._master
        f32 = lambda k: sd[k].to(dev).float().contiguous()
        lin = lambda k: sd[k].to(dev, dtp).contiguous()
        v = "vision_model"
        H, K = c["hidden_size"], 3 * c["patch_size"] ** 2
        wpe = torch.zeros(H, round_up(K, 8), device=dev, dtype=dtp)       # the conv weight as GEMM rows, K padded like emo_patch_rows' rows
        wpe[:, :K] = sd[f"{v}.embeddings.patch_embedding.weight"].reshape(H, K).to(dev, dtp)
        w = {"patch": wpe, "cls": lin(f"{v}.embeddings.class_embedding"), "pos": lin(f"{v}.embeddings.position_embedding.weight"),
             "pre.g": f32(f"{v}.pre_layrnorm.weight"), "pre.b": f32(f"{v}.pre_layrnorm.bias"),
             "post.g": f32(f"{v}.post_layernorm.weight"), "post.b": f32(f"{v}.post_layernorm.bias")}
        if self._projection:
            w["proj"] = lin("visual_projection.weight")
        w.update(pack_clip_layers(sd, f"{v}.encoder.layers", c["num_hidden_layers"], dev, dtp))
        return w

    # ---- forward
    def _check_inputs(self, pixel_values, output_attentions, interpolate_pos_encoding):
        if interpolate_pos_encoding:
            raise NotImplementedError(f"{self._name}: interpolate_pos_encoding is not built (the reference encodes at image_size)")
        if output_attentions:
            raise NotImplementedError(f"{self._name}: output_attentions is not built (the attention kernel never materialises the probabilities)")
        S = self._cfg["image_size"]
        if pixel_values is None or pixel_values.dim() != 4 or pixel_values.shape[1] != 3:
            raise ValueError("pixel_values must be (batch, 3, image_size, image_size)")
        if tuple(pixel_values.shape[2:]) != (S, S):
            raise ValueError(f"pixel_values are {tuple(pixel_values.shape[2:])}, the model takes image_size {S} x {S} (interpolate_pos_encoding is not built)")

    def _encode(self, pixel_values, output_hidden_states):
        """-> (last_hidden_state rows (B * L, H), pooler_output (B, H), [hidden states rows] or None, B, L)"""
        c, w, dev = self._cfg, self._w, self.device
        B = pixel_values.shape[0]
        H, eps, P = c["hidden_size"], c["layer_norm_eps"], c["patch_size"]
        L = (c["image_size"] // P) ** 2 + 1
        a = ops.patch_rows(pixel_values.detach().to(dev).float(), P, self.dtype)                  # (B*Np, r8(3 P P))
        h = ops.vision_embed(ops.gemm(a, w["patch"]), w["cls"], w["pos"], w["pre.g"], w["pre.b"], B, eps)     # (B*L, H) = hidden_states[0]
        hs = [h] if output_hidden_states else None
        h = run_clip_layers(h, w, n_layers=c["num_hidden_layers"], B=B, L=L, H=H, heads=c["num_attention_heads"], eps=eps,
                            act=_ACTS[c["hidden_act"]], causal=False, collect=hs)
        pooled = ops.layer_norm(h.view(B, L * H)[:, :H], w["post.g"], w["post.b"], eps)           # the class token of every image: a strided rows view
        return h, pooled, hs, B, L

    @torch.no_grad()
    def forward(self, pixel_values=None, output_attentions=False, output_hidden_states=False, interpolate_pos_encoding=False,
                return_dict=None, **_ignored):
        self._need()
        self._check_inputs(pixel_values, output_attentions, interpolate_pos_encoding)
        h, pooled, hs, B, L = self._encode(pixel_values, output_hidden_states)
        H = self._cfg["hidden_size"]
        hidden = tuple(t.view(B, L, H) for t in hs) if hs is not None else None
        if not self._projection:
            return CLIPVisionModelOutput(last_hidden_state=h.view(B, L, H), pooler_output=pooled, hidden_states=hidden)
        return CLIPVisionModelWithProjectionOutput(image_embeds=ops.gemm(pooled, self._w["proj"]), last_hidden_state=h.view(B, L, H),
                                                   pooler_output=pooled, hidden_states=hidden)


class CLIPVisionModelWithProjection(CLIPVisionModel):
    """forward(pixel_values) -> namespace(image_embeds (B, projection_dim), last_hidden_state, pooler_output, hidden_states); `[0]` is
    image_embeds, what the image-conditioned pipelines read."""
    _projection = True
    _name = "CLIPVisionModelWithProjection"
    _tolerated = frozenset({"vision_model.embeddings.position_ids"})


# ---------------------------------------------------------------------------------------------------------------- image processor
def resize_output_size(height, width, shortest_edge):
    """transformers get_resize_output_image_size(default_to_square=False): the shorter edge becomes `shortest_edge`, the longer one
    int(shortest_edge * long / short)."""
    short, long = (width, height) if width <= height else (height, width)
    new_short, new_long = int(shortest_edge), int(shortest_edge * long / short)
    return (new_long, new_short) if width <= height else (new_short, new_long)


def center_crop_offsets(height, width, crop):
    """transformers center_crop: (top, left) of the crop x crop window in a height x width image."""
    return (height - crop) // 2, (width - crop) // 2


def _aa_bicubic_taps(in_size, out_size, first, count):
    """Tap table of output indices [first, first + count) of an antialiased bicubic resize in_size -> out_size, in torch's arithmetic
    (aten UpSampleKernel `_compute_indices_min_size_weights_aa`, f32): scale = in / out, support = 2 * max(scale, 1), centre =
    scale * (i + 0.5), taps [int(centre - support + 0.5), int(centre + support + 0.5)) clipped to the image, weight
    keys((j - centre + 0.5) / max(scale, 1)) with a = -0.5, renormalised to sum 1.  -> (int32 (count, 2) = (first tap, taps), f32 (count, k))."""
    f = np.float32
    scale = f(in_size) / f(out_size)
    support = f(2.0) * scale if scale >= 1.0 else f(2.0)
    invscale = f(1.0) / scale if scale >= 1.0 else f(1.0)
    kmax = int(math.ceil(float(support))) * 2 + 1
    i = np.arange(first, first + count, dtype=np.float32)
    center = scale * (i + f(0.5))
    xmin = np.maximum((center - support + f(0.5)).astype(np.int64), 0)
    xsize = np.minimum(np.minimum((center + support + f(0.5)).astype(np.int64), in_size) - xmin, kmax)
    xsize = np.maximum(xsize, 0)
    j = np.arange(kmax, dtype=np.int64)[None, :]
    x = np.abs(((j + xmin[:, None]).astype(np.float32) - center[:, None] + f(0.5)) * invscale).astype(np.float32)
    a = f(-0.5)
    w1 = ((a + f(2.0)) * x - (a + f(3.0))) * x * x + f(1.0)
    w2 = ((a * x - f(5.0) * a) * x + f(8.0) * a) * x - f(4.0) * a
    wt = np.where(x < 1.0, w1, np.where(x < 2.0, w2, f(0.0))).astype(np.float32)
    wt = np.where(j < xsize[:, None], wt, f(0.0)).astype(np.float32)
    tot = wt.sum(1, dtype=np.float32)
    wt = np.where(tot[:, None] != 0, wt / np.where(tot == 0, f(1.0), tot)[:, None], wt).astype(np.float32)
    return np.stack([xmin, xsize], 1).astype(np.int32), wt


def resize_crop_taps(height, width, shortest_edge, crop):
    """Everything emo_image_preprocess needs for a height x width frame: -> dict(size=(rh, rw), top, left, ytap, yw, xtap, xw, span_max),
    numpy tables for the `crop` output rows / columns of the window."""
    rh, rw = resize_output_size(height, width, shortest_edge)
    top, left = center_crop_offsets(rh, rw, crop)
    if top < 0 or left < 0:
        raise ValueError(f"the {rh} x {rw} resized image is smaller than the {crop} x {crop} crop (zero padding is not built)")
    ytap, yw = _aa_bicubic_taps(height, rh, top, crop)
    xtap, xw = _aa_bicubic_taps(width, rw, left, crop)
    span = 1
    for o in range(0, crop, 64):          # the 64-column tiles of the kernel
        last = min(o + 64, crop) - 1
        span = max(span, int(xtap[last, 0] + xtap[last, 1] - xtap[o, 0]))
    return dict(size=(rh, rw), top=top, left=left, ytap=ytap, yw=yw, xtap=xtap, xw=xw, span_max=min(span, width))


class CLIPImageProcessor:
    """transformers' CLIPImageProcessor surface on emo_image_preprocess: `preprocess(images, return_tensors="pt")` / `__call__` ->
    namespace(pixel_values f32 (n, 3, crop, crop) on the device).  images: a PIL image, an (H, W, 3) uint8 array or tensor, a list of
    those, or an (n, H, W, 3) batch.  PIL only hands over an image object's bytes; resizing is the kernel's."""

    def __init__(self, size=None, crop_size=None, image_mean=None, image_std=None, rescale_factor=1 / 255, do_convert_rgb=True,
                 resample=3, do_resize=True, do_center_crop=True, do_rescale=True, do_normalize=True, device="cuda", **_ignored):
        size = {"shortest_edge": 224} if size is None else size
        if isinstance(size, dict):
            if set(size) != {"shortest_edge"}:
                raise NotImplementedError(f"CLIPImageProcessor: size {size} (only shortest_edge, CLIP's rule, is built)")
            size = size["shortest_edge"]
        crop_size = 224 if crop_size is None else crop_size
        if isinstance(crop_size, dict):
            if crop_size["height"] != crop_size["width"]:
                raise NotImplementedError("CLIPImageProcessor: a square crop_size")
            crop_size = crop_size["height"]
        if resample != 3:
            raise NotImplementedError("CLIPImageProcessor: resample must be bicubic (PIL.Image.BICUBIC = 3)")
        if not (do_resize and do_center_crop and do_rescale and do_normalize):
            raise NotImplementedError("CLIPImageProcessor: the resize, centre crop, rescale and normalise steps run as ONE kernel; none can be switched off")
        self.size, self.crop_size = {"shortest_edge": int(size)}, {"height": int(crop_size), "width": int(crop_size)}
        self.image_mean = list(OPENAI_CLIP_MEAN if image_mean is None else image_mean)
        self.image_std = list(OPENAI_CLIP_STD if image_std is None else image_std)
        self.rescale_factor, self.do_convert_rgb, self.resample = float(rescale_factor), bool(do_convert_rgb), 3
        self.device = torch.device(device)
        self._taps = {}     # (H, W) -> device tables

    def to(self, device):
        self.device, self._taps = torch.device(device), {}
        return self

    def _frames(self, images):
        """-> list of uint8 (n, H, W, 3) tensors, one per run of equal geometry, in input order"""
        def one(im):
            if hasattr(im, "convert") and hasattr(im, "size"):                  # a PIL image: only its bytes are taken
                im = np.array(im.convert("RGB") if self.do_convert_rgb else im)
            t = torch.as_tensor(im)
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
                raise ValueError(f"an image must be (H, W, 3) uint8 RGB, got {tuple(t.shape)} {t.dtype}")
            return t
        if torch.is_tensor(images) or isinstance(images, np.ndarray):
            t = torch.as_tensor(images)
            if t.dim() == 4:
                if t.dtype != torch.uint8 or t.shape[3] != 3:
                    raise ValueError(f"a batch must be (n, H, W, 3) uint8 RGB, got {tuple(t.shape)} {t.dtype}")
                return [t]
            return [one(t)[None]]
        if not isinstance(images, (list, tuple)):
            return [one(images)[None]]
        if not images:
            raise ValueError("no images")
        out = []
        for t in map(one, images):
            if out and out[-1][0].shape == t.shape:
                out[-1].append(t)
            else:
                out.append([t])
        return [torch.stack(g) for g in out]

    def _tables(self, H, W):
        if (H, W) not in self._taps:
            t = resize_crop_taps(H, W, self.size["shortest_edge"], self.crop_size["height"])
            dev = self.device
            self._taps[(H, W)] = tuple(torch.from_numpy(np.ascontiguousarray(t[k])).to(dev) for k in ("ytap", "yw", "xtap", "xw")) + (t["span_max"],)
        return self._taps[(H, W)]

    @torch.no_grad()
    def preprocess(self, images, return_tensors="pt", **_ignored):
        if return_tensors not in (None, "pt"):
            raise NotImplementedError("CLIPImageProcessor: return_tensors='pt' (the pixel values stay on the device)")
        if self.device.type != "cuda":
            raise EmoHipError("CLIPImageProcessor: emo_image_preprocess runs on a HIP device (there is no CPU execution path)")
        S, outs = self.crop_size["height"], []
        for fr in self._frames(images):
            ytap, yw, xtap, xw, span = self._tables(fr.shape[1], fr.shape[2])
            outs.append(ops.image_preprocess(fr.contiguous().to(self.device), S, ytap, yw, xtap, xw, span, self.rescale_factor, self.image_mean,
                                             self.image_std))
        return SimpleNamespace(pixel_values=outs[0] if len(outs) == 1 else torch.cat(outs))

    __call__ = preprocess
