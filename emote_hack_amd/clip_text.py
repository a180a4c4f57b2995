"""The CLIP text encoder of the reference on MI355X: `_encode_prompt` (EMOAnimationPipeline.py:202-289) calls
`CLIPTextModel(input_ids)[0]`, the transformers model magicanimate/pipelines/animation.py:75-76,98 loads in fp16 (SD-1.5's
`text_encoder`).  Third-party, weights from the network, so weights are CALLER-LOADED here (`load_state_dict` takes transformers' key
names, `from_pretrained` reads a local checkpoint folder); the tokenizer stays the caller's (its vocabulary is downloaded data).

  embeddings   emo_text_embed: token + position embedding in one launch (ids range-checked on the host, IndexError like nn.Embedding)
  12 layers    pre-LN: LN1 folded into the q | k projection and into the V^T projection (two launches: the split V^T store of one launch
               needs M % 32 == 0, and 2 x 77 rows are not), emo_attention with the causal mask (12 heads of 64), out_proj + residual,
               LN2 folded into fc1, emo_act quick_gelu, fc2 + residual
  final LN     emo_layernorm; pooler_output = the EOS row of each sequence (host-side index from the CPU ids, emo_gather_rows)

Pinned by outputs of transformers' own CLIPTextModel (tools/oracle/gen_golden_clip.py -> tests/golden/clip_text.safetensors).
Not built: key-padding masks, non-default position_ids, clip-skip (output_hidden_states) - the reference uses none of them.
"""
from __future__ import annotations

import json
import os
from types import SimpleNamespace

import torch

from . import ops
from ._lib import EmoHipError
from .synth import synth_state_dict

# SD-1.5's text_encoder/config.json (openai/clip-vit-large-patch14's text tower); eos_token_id 2 is what that legacy file says
# (pooling then takes the argmax of the ids - transformers CLIPTextTransformer keeps that rule for such configs)
SD15_CONFIG = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                   max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, bos_token_id=0, eos_token_id=2,
                   pad_token_id=1)
_ACTS = {"quick_gelu": "quick_gelu", "gelu": "gelu"}


def _r8(x):
    return (x + 7) // 8 * 8


def clip_text_param_shapes(cfg=None):
    """transformers' CLIPTextModel state-dict keys / shapes (without the non-persistent `position_ids` buffer)."""
    c = dict(SD15_CONFIG, **(cfg or {}))
    H, I, P = c["hidden_size"], c["intermediate_size"], c["max_position_embeddings"]
    d = {"text_model.embeddings.token_embedding.weight": (c["vocab_size"], H),
         "text_model.embeddings.position_embedding.weight": (P, H)}
    for i in range(c["num_hidden_layers"]):
        p = f"text_model.encoder.layers.{i}"
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            d[f"{p}.self_attn.{n}.weight"] = (H, H)
            d[f"{p}.self_attn.{n}.bias"] = (H,)
        d[f"{p}.layer_norm1.weight"] = (H,)
        d[f"{p}.layer_norm1.bias"] = (H,)
        d[f"{p}.mlp.fc1.weight"] = (I, H)
        d[f"{p}.mlp.fc1.bias"] = (I,)
        d[f"{p}.mlp.fc2.weight"] = (H, I)
        d[f"{p}.mlp.fc2.bias"] = (H,)
        d[f"{p}.layer_norm2.weight"] = (H,)
        d[f"{p}.layer_norm2.bias"] = (H,)
    d["text_model.final_layer_norm.weight"] = (H,)
    d["text_model.final_layer_norm.bias"] = (H,)
    return d


def clip_text_synth_state_dict(cfg=None, prefix="clip_text.", device="cpu"):
    """Name-keyed synthetic weights (emote_hack_amd.synth) under transformers' key names."""
    return synth_state_dict(clip_text_param_shapes(cfg), prefix=prefix, device=device)


class CLIPTextModel:
    """forward(input_ids (B, L) with L <= max_position_embeddings) -> namespace(last_hidden_state (B, L, hidden), pooler_output (B, hidden))
    in the model's dtype; `[0]` is last_hidden_state, like the transformers output `_encode_prompt` indexes (EMOAnimationPipeline.py:226-229)."""

    def __init__(self, config=None, **kwargs):
        cfg = dict(SD15_CONFIG)
        if config is not None:
            cfg.update(config if isinstance(config, dict) else {k: getattr(config, k) for k in SD15_CONFIG if hasattr(config, k)})
        cfg.update(kwargs)
        cfg = {k: cfg[k] for k in SD15_CONFIG}
        if cfg["hidden_act"] not in _ACTS:
            raise NotImplementedError(f"CLIPTextModel: hidden_act {cfg['hidden_act']!r} (quick_gelu | gelu)")
        H, nh = cfg["hidden_size"], cfg["num_attention_heads"]
        if H % nh or (H // nh) % 8 or cfg["intermediate_size"] % 8:
            raise ValueError("CLIPTextModel: the head dim and the widths must be multiples of 8")
        self.config = SimpleNamespace(**cfg)
        self._cfg = cfg
        self._shapes = clip_text_param_shapes(cfg)
        self._sd, self._w = None, None
        self.dtype, self.device = torch.float32, torch.device("cpu")

    @classmethod
    def from_pretrained(cls, pretrained_model_path, subfolder="text_encoder", torch_dtype=None, **_ignored):
        """A LOCAL checkpoint folder (`<path>/<subfolder>/config.json` + `model.safetensors` or `pytorch_model.bin`), as
        animation.py:75-76 names it - nothing is fetched."""
        path = os.path.join(pretrained_model_path, subfolder) if subfolder else pretrained_model_path
        config_file = os.path.join(path, "config.json")
        if not os.path.isfile(config_file):
            raise RuntimeError(f"{config_file} does not exist")
        with open(config_file) as f:
            config = json.load(f)
        model = cls({k: config[k] for k in SD15_CONFIG if k in config})
        st_file, bin_file = os.path.join(path, "model.safetensors"), os.path.join(path, "pytorch_model.bin")
        if os.path.isfile(st_file):
            from safetensors.torch import load_file
            sd = load_file(st_file)
        elif os.path.isfile(bin_file):
            sd = torch.load(bin_file, map_location="cpu", weights_only=True)
        else:
            raise RuntimeError(f"neither {st_file} nor {bin_file} exists")
        model.load_state_dict(sd)
        if torch_dtype is not None:
            model.to(dtype=torch_dtype)
        return model

    # ---- torch-module-like surface
    def eval(self):
        return self

    def requires_grad_(self, _flag=True):
        return self

    def state_dict(self):
        if self._sd is None:
            raise EmoHipError("no weights loaded")
        return dict(self._sd)

    def load_state_dict(self, sd, strict=True):
        sd = dict(sd)
        # older SD-1.5 checkpoints carry the position_ids buffer; transformers ignores it (non-persistent)
        tolerated = {"text_model.embeddings.position_ids"}
        missing = [k for k in self._shapes if k not in sd]
        unexpected = [k for k in sd if k not in self._shapes and k not in tolerated]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: {len(missing)} missing {missing[:4]}, {len(unexpected)} unexpected {unexpected[:4]}")
        for k, shp in self._shapes.items():
            if k in sd and tuple(sd[k].shape) != tuple(shp):
                raise RuntimeError(f"size mismatch for {k}: {tuple(sd[k].shape)} vs {tuple(shp)}")
        self._sd = {k: sd[k].detach().float() for k in self._shapes if k in sd}
        self._pack()
        return missing, unexpected

    def to(self, *args, **kwargs):
        device, dtype = kwargs.get("device"), kwargs.get("dtype")
        for a in args:
            if isinstance(a, torch.dtype):
                dtype = a
            else:
                device = torch.device(a)
        if dtype is not None:
            ops.dt(dtype)
            self.dtype = dtype
        if device is not None:
            self.device = torch.device(device)
        self._pack()
        return self

    def _pack(self):
        if self._sd is None or self.device.type != "cuda" or any(k not in self._sd for k in self._shapes):
            return
        c, dev, dtp, sd = self._cfg, self.device, self.dtype, self._sd
        f32 = lambda k: sd[k].to(dev).float().contiguous()
        lin = lambda k: sd[k].to(dev, dtp).contiguous()

        def ln_fold(wt, b, norm):
            """(W, b) of a Linear behind LayerNorm `norm` -> (W * gamma in the compute dtype, its row sums, b + W . beta):
            LN(x) W^T + b = rstd (x W'^T - mean colsum) + b' (the UNet's fold, emo_gemm_params.ln_colsum)."""
            g_, be = sd[norm + ".weight"].to(dev).float(), sd[norm + ".bias"].to(dev).float()
            wt = wt.to(dev).float()
            wp = (wt * g_[None, :]).to(dtp)
            bp = wt.to(dtp).float() @ be + b.to(dev).float()
            return wp.contiguous(), wp.float().sum(1).contiguous(), bp.contiguous()

        w = {"tok": lin("text_model.embeddings.token_embedding.weight"), "pos": lin("text_model.embeddings.position_embedding.weight"),
             "lnf.g": f32("text_model.final_layer_norm.weight"), "lnf.b": f32("text_model.final_layer_norm.bias")}
        for i in range(c["num_hidden_layers"]):
            p = f"text_model.encoder.layers.{i}.self_attn"
            w[f"{i}.qk"] = ln_fold(torch.cat([sd[f"{p}.q_proj.weight"], sd[f"{p}.k_proj.weight"]]),
                                   torch.cat([sd[f"{p}.q_proj.bias"], sd[f"{p}.k_proj.bias"]]), f"text_model.encoder.layers.{i}.layer_norm1")
            w[f"{i}.v"] = ln_fold(sd[f"{p}.v_proj.weight"], sd[f"{p}.v_proj.bias"], f"text_model.encoder.layers.{i}.layer_norm1")
            w[f"{i}.o.w"], w[f"{i}.o.b"] = lin(f"{p}.out_proj.weight"), f32(f"{p}.out_proj.bias")
            m = f"text_model.encoder.layers.{i}.mlp"
            w[f"{i}.f1"] = ln_fold(sd[f"{m}.fc1.weight"], sd[f"{m}.fc1.bias"], f"text_model.encoder.layers.{i}.layer_norm2")
            w[f"{i}.f2.w"], w[f"{i}.f2.b"] = lin(f"{m}.fc2.weight"), f32(f"{m}.fc2.bias")
        self._w = w

    # ---- forward
    def _check_inputs(self, input_ids, attention_mask, position_ids, output_hidden_states, output_attentions):
        if output_hidden_states or output_attentions:
            raise NotImplementedError("CLIPTextModel: output_hidden_states / output_attentions (clip-skip) are not built - "
                                      "_encode_prompt reads [0] only (EMOAnimationPipeline.py:229)")
        if input_ids is None or input_ids.dim() != 2:
            raise ValueError("input_ids must be (batch, seq_len)")
        B, L = input_ids.shape
        if L < 1 or L > self._cfg["max_position_embeddings"]:
            raise ValueError(f"sequence length {L} must lie in [1, {self._cfg['max_position_embeddings']}] (max_position_embeddings)")
        if attention_mask is not None and bool((torch.as_tensor(attention_mask).cpu() == 0).any()):
            raise NotImplementedError("CLIPTextModel: key-padding attention masks are not built (SD-1.5's text encoder is called without one, "
                                      "EMOAnimationPipeline.py:220-224); an all-ones mask is accepted")
        if position_ids is not None:
            pid = torch.as_tensor(position_ids).cpu()
            if not torch.equal(pid.expand(B, L) if pid.dim() == 2 else pid.reshape(1, -1).expand(B, L),
                               torch.arange(L).expand(B, L).to(pid.dtype)):
                raise NotImplementedError("CLIPTextModel: only the default position_ids (arange(seq_len)) are built")

    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, output_hidden_states=False, output_attentions=False,
                return_dict=None, **_ignored):
        if self._w is None:
            raise EmoHipError("CLIPTextModel: load_state_dict + .to('cuda') first (weights are caller-loaded; there is no CPU execution path)")
        self._check_inputs(input_ids, attention_mask, position_ids, output_hidden_states, output_attentions)
        c, w, dev = self._cfg, self._w, self.device
        ids = input_ids.detach().cpu().to(torch.int64)
        B, L = ids.shape
        H, nh, eps = c["hidden_size"], c["num_attention_heads"], c["layer_norm_eps"]
        d = H // nh
        act = _ACTS[c["hidden_act"]]
        h = ops.text_embed(ids, w["tok"], w["pos"])                                               # (B*L, H)
        for i in range(c["num_hidden_layers"]):
            st = ops.layer_norm_stats(h, eps)
            wq, cs, bq = w[f"{i}.qk"]
            qk = ops.gemm(h, wq, bq, ln=(cs, st))                                                 # LN1 -> q | k
            wv, cs, bv = w[f"{i}.v"]
            vt = ops.gemm(h, wv, bv, ln=(cs, st), transpose_rows=L, transpose_ld=_r8(L))          # LN1 -> V^T (B, H, ld)
            att = ops.attention(qk[:, :H], qk[:, H:], vt, L, B=B, Lq=L, heads=nh, d=d, scale=d ** -0.5, causal=True)
            h = ops.gemm(att, w[f"{i}.o.w"], w[f"{i}.o.b"], residual=h)
            st = ops.layer_norm_stats(h, eps)
            w1, cs, b1 = w[f"{i}.f1"]
            f = ops.act(ops.gemm(h, w1, b1, ln=(cs, st)), act)                                    # LN2 -> fc1 -> activation
            h = ops.gemm(f, w[f"{i}.f2.w"], w[f"{i}.f2.b"], residual=h)
        h = ops.layer_norm(h, w["lnf.g"], w["lnf.b"], eps)
        # pooling (transformers CLIPTextTransformer): the legacy eos_token_id 2 takes the argmax of the ids, otherwise the first EOS
        if c["eos_token_id"] == 2:
            pos = ids.to(torch.int).argmax(dim=-1)
        else:
            pos = (ids.to(torch.int) == c["eos_token_id"]).int().argmax(dim=-1)
        rows = (torch.arange(B) * L + pos).to(torch.int32).to(dev)
        pooled = ops.gather_rows(h, rows)
        return CLIPTextModelOutput(last_hidden_state=h.view(B, L, H), pooler_output=pooled)

    __call__ = forward


class CLIPTextModelOutput(SimpleNamespace):
    """transformers' BaseModelOutputWithPooling surface: `.last_hidden_state`, `.pooler_output`, and `[0]` / `[1]` in that order."""

    def __getitem__(self, i):
        return (self.last_hidden_state, self.pooler_output)[i]
