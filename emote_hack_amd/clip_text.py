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

from types import SimpleNamespace

import torch

from . import ops
from .clip_layers import ACTS as _ACTS, clip_layer_shapes, load_local_checkpoint, pack_clip_layers, run_clip_layers
from .module import HipModule
from .synth import synth_state_dict

# SD-1.5's text_encoder/config.json (openai/clip-vit-large-patch14's text tower); eos_token_id 2 is what that legacy file says
# (pooling then takes the argmax of the ids - transformers CLIPTextTransformer keeps that rule for such configs)
SD15_CONFIG = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                   max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, bos_token_id=0, eos_token_id=2,
                   pad_token_id=1)


def clip_text_param_shapes(cfg=None):
    """transformers' CLIPTextModel state-dict keys / shapes (without the non-persistent `position_ids` buffer)."""
    c = dict(SD15_CONFIG, **(cfg or {}))
    H, I, P = c["hidden_size"], c["intermediate_size"], c["max_position_embeddings"]
    d = {"text_model.embeddings.token_embedding.weight": (c["vocab_size"], H),
         "text_model.embeddings.position_embedding.weight": (P, H)}
    d.update(clip_layer_shapes("text_model.encoder.layers", c["num_hidden_layers"], H, I))
    d["text_model.final_layer_norm.weight"] = (H,)
    d["text_model.final_layer_norm.bias"] = (H,)
    return d


def clip_text_synth_state_dict(cfg=None, prefix="clip_text.", device="cpu"):
    """Name-keyed synthetic weights (emote_hack_amd.synth) under transformers' key names."""
    return synth_state_dict(clip_text_param_shapes(cfg), prefix=prefix, device=device)


class CLIPTextModel(HipModule):
    """forward(input_ids (B, L) with L <= max_position_embeddings) -> namespace(last_hidden_state (B, L, hidden), pooler_output (B, hidden))
    in the model's dtype; `[0]` is last_hidden_state, like the transformers output `_encode_prompt` indexes (EMOAnimationPipeline.py:226-229)."""
    # older SD-1.5 checkpoints carry the position_ids buffer; transformers ignores it (non-persistent)
    _tolerated = frozenset({"text_model.embeddings.position_ids"})

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
        super().__init__(clip_text_param_shapes(cfg))

    @classmethod
    def from_pretrained(cls, pretrained_model_path, subfolder="text_encoder", torch_dtype=None, **_ignored):
        """A LOCAL checkpoint folder (`<path>/<subfolder>/config.json` + `model.safetensors` or `pytorch_model.bin`), as
        animation.py:75-76 names it - nothing is fetched."""
        config, sd = load_local_checkpoint(pretrained_model_path, subfolder)
        model = cls({k: config[k] for k in SD15_CONFIG if k in config})
        model.load_state_dict(sd)
        if torch_dtype is not None:
            model.to(dtype=torch_dtype)
        return model

    def _pack_weights(self):
        c, dev, dtp, sd = self._cfg, self.device, self.dtype, self._master
        f32 = lambda k: sd[k].to(dev).float().contiguous()
        lin = lambda k: sd[k].to(dev, dtp).contiguous()
        w = {"tok": lin("text_model.embeddings.token_embedding.weight"), "pos": lin("text_model.embeddings.position_embedding.weight"),
             "lnf.g": f32("text_model.final_layer_norm.weight"), "lnf.b": f32("text_model.final_layer_norm.bias")}
        w.update(pack_clip_layers(sd, "text_model.encoder.layers", c["num_hidden_layers"], dev, dtp))
        return w

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
        self._need()
        self._check_inputs(input_ids, attention_mask, position_ids, output_hidden_states, output_attentions)
        c, w, dev = self._cfg, self._w, self.device
        ids = input_ids.detach().cpu().to(torch.int64)
        B, L = ids.shape
        H = c["hidden_size"]
        h = ops.text_embed(ids, w["tok"], w["pos"])                                               # (B*L, H)
        h = run_clip_layers(h, w, n_layers=c["num_hidden_layers"], B=B, L=L, H=H, heads=c["num_attention_heads"],
                            eps=c["layer_norm_eps"], act=_ACTS[c["hidden_act"]], causal=True)
        h = ops.layer_norm(h, w["lnf.g"], w["lnf.b"], c["layer_norm_eps"])
        # pooling (transformers CLIPTextTransformer): the legacy eos_token_id 2 takes the argmax of the ids, otherwise the first EOS
        if c["eos_token_id"] == 2:
            pos = ids.to(torch.int).argmax(dim=-1)
        else:
            pos = (ids.to(torch.int) == c["eos_token_id"]).int().argmax(dim=-1)
        rows = (torch.arange(B) * L + pos).to(torch.int32).to(dev)
        pooled = ops.gather_rows(h, rows)
        return CLIPTextModelOutput(last_hidden_state=h.view(B, L, H), pooler_output=pooled)


class CLIPTextModelOutput(SimpleNamespace):
    """transformers' BaseModelOutputWithPooling surface: `.last_hidden_state`, `.pooler_output`, and `[0]` / `[1]` in that order."""

    def __getitem__(self, i):
        return (self.last_hidden_state, self.pooler_output)[i]
