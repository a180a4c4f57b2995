"""The audio front-end of the reference on MI355X: the wav2vec2 encoder and the feature extractor around it.

  Wav2Vec2Model           the network `Wav2VecFeatureExtractor.__init__` loads (Net.py:607-612: transformers'
                          `Wav2Vec2Model.from_pretrained('facebook/wav2vec2-base-960h')`) - third-party, weights from the network,
                          so weights are CALLER-LOADED here (`load_state_dict` takes transformers' key names); the forward runs on
                          the kernels the UNet already uses:
                            feature encoder   7 strided Conv1d layers = GEMMs over an overlapping ROW VIEW of the (time, channel)
                                              activation (window t of kernel k / stride s is k*C contiguous elements at row t*s:
                                              lda = s*C, K = k*C - no im2col copy), emo_channelnorm (+GELU) behind layer 0, emo_act GELU
                            projection        emo_layernorm + emo_gemm
                            positional conv   16 per-group GEMMs over the same kind of row view (k = 128), GELU, residual
                            12 layers         emo_gemm (q | k fused, V^T by the transposed store) + emo_attention (12 heads of 64) +
                                              emo_layernorm + GELU feed-forward
                          The wav2vec2-large family (wav2vec2-large-960h-lv60, large-xlsr-53, XLS-R, large-robust: LARGE_CONFIG) differs
                          by three config switches, each served on its own:
                            feat_extract_norm "layer"   every conv is conv (+ bias) -> LayerNorm(C) -> GELU per time step: layer 0 by
                                              emo_wav_conv0_ln_act straight from the waveform (or the window-matrix GEMM + emo_layernorm_act:
                                              `conv0_route`), layers 1-6 a row-view GEMM + bias and emo_layernorm_act
                            conv_bias         the bias rides in the GEMM epilogue
                            do_stable_layer_norm   pre-LN layers = clip_layers.run_clip_layers (LayerNorms folded into the q | k, V^T and
                                              fc1 GEMMs) over a key-renaming view of the master dict, encoder.layer_norm last
                          and its processor returns an attention_mask: forward takes right-padded batches with one (see forward).
  Wav2VecFeatureExtractor extract_features_from_wav behind the file read (Net.py:636-667): utterance normalisation (what
                          `self.processor(...)` does), encoder, emo_audio_windows -> (T, (m + n + 1) * 768)

Oracle: oracle/wav2vec2_ref.py, pinned by outputs of transformers' own model (tests/golden/wav2vec2.safetensors).
Both checkpoint families are built: wav2vec2-base (feat_extract_norm "group", post-LN encoder - the one the reference names) and
wav2vec2-large (feat_extract_norm "layer", conv biases, pre-LN encoder; goldens tests/golden/wav2vec2_large.safetensors from
tools/oracle/gen_golden_wav2vec2_large.py).
"""
from __future__ import annotations

import os
from types import SimpleNamespace

import torch

from . import ops
from .clip_layers import load_local_checkpoint, pack_clip_layers, run_clip_layers
from .module import HipModule, round_up
from .synth import synth_state_dict, synth_tensor

BASE_CONFIG = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                   conv_dim=(512, 512, 512, 512, 512, 512, 512), conv_stride=(5, 2, 2, 2, 2, 2, 2), conv_kernel=(10, 3, 3, 3, 3, 2, 2),
                   conv_bias=False, feat_extract_norm="group", num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16,
                   do_stable_layer_norm=False, layer_norm_eps=1e-5)
# wav2vec2-large-960h-lv60(-self), wav2vec2-large-xlsr-53, the XLS-R models, wav2vec2-large-robust
LARGE_CONFIG = dict(BASE_CONFIG, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, conv_bias=True,
                    feat_extract_norm="layer", do_stable_layer_norm=True)


def wav2vec2_param_shapes(cfg=None):
    """transformers' Wav2Vec2Model state-dict keys / shapes for a config (parametrised weight-norm spelling): conv biases with
    `conv_bias`, a LayerNorm behind every conv with feat_extract_norm "layer" (behind layer 0 only - a GroupNorm - with "group").  The
    encoder's keys are the same for the post-LN and the pre-LN (`do_stable_layer_norm`) layers."""
    c = dict(BASE_CONFIG, **(cfg or {}))
    d, cin = {}, 1
    for i, (co, k) in enumerate(zip(c["conv_dim"], c["conv_kernel"])):
        d[f"feature_extractor.conv_layers.{i}.conv.weight"] = (co, cin, k)
        if c["conv_bias"]:
            d[f"feature_extractor.conv_layers.{i}.conv.bias"] = (co,)
        if c["feat_extract_norm"] == "layer":
            d[f"feature_extractor.conv_layers.{i}.layer_norm.weight"] = (co,)
            d[f"feature_extractor.conv_layers.{i}.layer_norm.bias"] = (co,)
        elif i == 0:
            d["feature_extractor.conv_layers.0.layer_norm.weight"] = (co,)
            d["feature_extractor.conv_layers.0.layer_norm.bias"] = (co,)
        cin = co
    H, I = c["hidden_size"], c["intermediate_size"]
    d["feature_projection.layer_norm.weight"] = (cin,)
    d["feature_projection.layer_norm.bias"] = (cin,)
    d["feature_projection.projection.weight"] = (H, cin)
    d["feature_projection.projection.bias"] = (H,)
    kp, g = c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"]
    d["encoder.pos_conv_embed.conv.bias"] = (H,)
    d["encoder.pos_conv_embed.conv.parametrizations.weight.original0"] = (1, 1, kp)
    d["encoder.pos_conv_embed.conv.parametrizations.weight.original1"] = (H, H // g, kp)
    d["encoder.layer_norm.weight"] = (H,)
    d["encoder.layer_norm.bias"] = (H,)
    for i in range(c["num_hidden_layers"]):
        p = f"encoder.layers.{i}"
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            d[f"{p}.attention.{n}.weight"] = (H, H)
            d[f"{p}.attention.{n}.bias"] = (H,)
        d[f"{p}.layer_norm.weight"] = (H,)
        d[f"{p}.layer_norm.bias"] = (H,)
        d[f"{p}.feed_forward.intermediate_dense.weight"] = (I, H)
        d[f"{p}.feed_forward.intermediate_dense.bias"] = (I,)
        d[f"{p}.feed_forward.output_dense.weight"] = (H, I)
        d[f"{p}.feed_forward.output_dense.bias"] = (H,)
        d[f"{p}.final_layer_norm.weight"] = (H,)
        d[f"{p}.final_layer_norm.bias"] = (H,)
    return d


def wav2vec2_synth_state_dict(cfg=None, prefix="wav2vec2.", device="cpu"):
    """Name-keyed synthetic weights (emote_hack_amd.synth) for the encoder; the weight-norm magnitude g is drawn around 3 so that the
    positional convolution is numerically visible (a fan-in scaled g would leave only its bias)."""
    sd = synth_state_dict(wav2vec2_param_shapes(cfg), prefix=prefix, device=device)
    k = "encoder.pos_conv_embed.conv.parametrizations.weight.original0"
    sd[k] = 3.0 * synth_tensor(prefix + k + ".g", sd[k].shape[-1:], device=device).reshape(sd[k].shape)     # 3 * (1 + 0.1 N(0,1))
    return sd


class _ClipLayerKeys:
    """The master dict under transformers' CLIPEncoderLayer key names, which clip_layers.pack_clip_layers reads: a pre-LN wav2vec2
    layer is that layer with other names (a view - nothing is copied)."""
    _RENAMES = (("self_attn.", "attention."), ("layer_norm1.", "layer_norm."), ("layer_norm2.", "final_layer_norm."),
                ("mlp.fc1.", "feed_forward.intermediate_dense."), ("mlp.fc2.", "feed_forward.output_dense."))

    def __init__(self, sd):
        self._sd = sd

    def __getitem__(self, key):
        for clip, own in self._RENAMES:
            if clip in key:
                return self._sd[key.replace(clip, own)]
        return self._sd[key]


class Wav2Vec2Model(HipModule):
    """forward(input_values (B, n_samples) f32) -> namespace(last_hidden_state=(B, T, hidden) f32), like the transformers class the
    reference calls (Net.py:643-644).  `conv0_route` ("fused" | "gemm") selects how layer 0 of a feat_extract_norm "layer" model runs:
    emo_wav_conv0_ln_act straight from the waveform, or the window-matrix GEMM + emo_layernorm_act (also the fallback for a first
    layer the fused kernel does not serve); forward(conv0_route=) overrides it for one call."""
    _tolerated = frozenset({"masked_spec_embed"})
    # keys of the Wav2Vec2ForCTC / Wav2Vec2ForPreTraining files the encoder has no use for
    _tolerated_prefixes = ("lm_head.", "quantizer.", "project_hid.", "project_q.")
    CONV0_ROUTES = ("fused", "gemm")

    def __init__(self, config=None, **kwargs):
        cfg = dict(BASE_CONFIG)
        if config is not None:
            cfg.update({k: getattr(config, k) for k in BASE_CONFIG if hasattr(config, k)} if not isinstance(config, dict) else config)
        cfg.update(kwargs)
        if cfg["feat_extract_norm"] not in ("group", "layer"):
            raise ValueError(f"Wav2Vec2Model: feat_extract_norm={cfg['feat_extract_norm']!r} must be 'group' or 'layer'")
        H, nh = cfg["hidden_size"], cfg["num_attention_heads"]
        if H % nh or (H // nh) % 8 or (H // cfg["num_conv_pos_embedding_groups"]) % 8 or any(c % 8 for c in cfg["conv_dim"]):
            raise ValueError("Wav2Vec2Model: head dim, positional-conv group width and conv channels must be multiples of 8")
        self.config = SimpleNamespace(**cfg)
        self._cfg = cfg
        self.conv0_route = "fused"
        super().__init__(wav2vec2_param_shapes(cfg))

    @classmethod
    def from_pretrained(cls, pretrained_model_path, subfolder=None, torch_dtype=None, **_ignored):
        """A LOCAL checkpoint folder (`<path>[/<subfolder>]/config.json` + `model.safetensors` or `pytorch_model.bin`) - nothing is
        fetched.  The family is read from config.json; Wav2Vec2ForCTC / ForPreTraining files load too (see _remap_keys)."""
        config, sd = load_local_checkpoint(pretrained_model_path, subfolder)
        model = cls({k: config[k] for k in BASE_CONFIG if k in config})
        model.load_state_dict(sd)
        if torch_dtype is not None:
            model.to(dtype=torch_dtype)
        return model

    def _remap_keys(self, sd):
        if any(k.startswith("wav2vec2.") for k in sd):        # a task model's file: the encoder under `wav2vec2.`, heads beside it
            sd = {(k[len("wav2vec2."):] if k.startswith("wav2vec2.") else k): v for k, v in sd.items()}
        for k in [k for k in sd if k.startswith(self._tolerated_prefixes)]:
            del sd[k]
        pc = "encoder.pos_conv_embed.conv."
        for old, new in ((pc + "weight_g", pc + "parametrizations.weight.original0"), (pc + "weight_v", pc + "parametrizations.weight.original1")):
            if old in sd and new not in sd:       # checkpoints written before torch's parametrised weight_norm
                sd[new] = sd.pop(old)
        return sd

    def _pack_weights(self):
        c, dev, dtp, sd = self._cfg, self.device, self.dtype, self._master
        w = {}
        f32 = lambda k: sd[k].to(dev).float().contiguous()
        lin = lambda k: sd[k].to(dev, dtp).contiguous()
        for i, k in enumerate(c["conv_kernel"]):
            t = sd[f"feature_extractor.conv_layers.{i}.conv.weight"]              # (Cout, Cin, k) -> [Cout][k][Cin]
            t = t.permute(0, 2, 1).reshape(t.shape[0], -1)
            if i == 0:       # Cin = 1: the k taps padded to a 16-byte multiple (the window matrix is padded alike)
                t = torch.nn.functional.pad(t, (0, round_up(k, 8) - k))
            w[f"conv{i}"] = t.to(dev, dtp).contiguous()
            w[f"conv{i}.b"] = f32(f"feature_extractor.conv_layers.{i}.conv.bias") if c["conv_bias"] else None
        if c["feat_extract_norm"] == "layer":
            for i in range(len(c["conv_kernel"])):
                w[f"cln{i}.g"] = f32(f"feature_extractor.conv_layers.{i}.layer_norm.weight")
                w[f"cln{i}.b"] = f32(f"feature_extractor.conv_layers.{i}.layer_norm.bias")
            # the fused first layer reads the f32 master taps (C, k), and a bias even where the checkpoint has none
            w["conv0.f32"] = f32("feature_extractor.conv_layers.0.conv.weight").reshape(c["conv_dim"][0], -1).contiguous()
            w["conv0.b32"] = w["conv0.b"] if c["conv_bias"] else torch.zeros(c["conv_dim"][0], device=dev, dtype=torch.float32)
        else:
            w["gn.g"], w["gn.b"] = f32("feature_extractor.conv_layers.0.layer_norm.weight"), f32("feature_extractor.conv_layers.0.layer_norm.bias")
        w["fp.ln.g"], w["fp.ln.b"] = f32("feature_projection.layer_norm.weight"), f32("feature_projection.layer_norm.bias")
        w["fp.w"], w["fp.b"] = lin("feature_projection.projection.weight"), f32("feature_projection.projection.bias")
        # weight_norm(dim=2): w = g * v / ||v||, the norm over every dim but 2 - formed once at load in f32
        g = sd["encoder.pos_conv_embed.conv.parametrizations.weight.original0"]
        v = sd["encoder.pos_conv_embed.conv.parametrizations.weight.original1"]
        wp = v * (g / v.norm(dim=(0, 1), keepdim=True))                           # (H, H/groups, k)
        G = c["num_conv_pos_embedding_groups"]
        cg = wp.shape[0] // G
        w["pos.w"] = [wp[gi * cg:(gi + 1) * cg].permute(0, 2, 1).reshape(cg, -1).to(dev, dtp).contiguous() for gi in range(G)]
        w["pos.b"] = [f32("encoder.pos_conv_embed.conv.bias")[gi * cg:(gi + 1) * cg].contiguous() for gi in range(G)]
        w["enc.ln.g"], w["enc.ln.b"] = f32("encoder.layer_norm.weight"), f32("encoder.layer_norm.bias")
        if c["do_stable_layer_norm"]:       # pre-LN: CLIP's layer under other key names
            w["layers"] = pack_clip_layers(_ClipLayerKeys(sd), "encoder.layers", c["num_hidden_layers"], dev, dtp)
            return w
        for i in range(c["num_hidden_layers"]):
            p = f"encoder.layers.{i}"
            w[f"{i}.qk.w"] = torch.cat([sd[f"{p}.attention.q_proj.weight"], sd[f"{p}.attention.k_proj.weight"]]).to(dev, dtp).contiguous()
            w[f"{i}.qk.b"] = torch.cat([sd[f"{p}.attention.q_proj.bias"], sd[f"{p}.attention.k_proj.bias"]]).to(dev).float().contiguous()
            w[f"{i}.v.w"], w[f"{i}.v.b"] = lin(f"{p}.attention.v_proj.weight"), f32(f"{p}.attention.v_proj.bias")
            w[f"{i}.o.w"], w[f"{i}.o.b"] = lin(f"{p}.attention.out_proj.weight"), f32(f"{p}.attention.out_proj.bias")
            w[f"{i}.ln1.g"], w[f"{i}.ln1.b"] = f32(f"{p}.layer_norm.weight"), f32(f"{p}.layer_norm.bias")
            w[f"{i}.f1.w"], w[f"{i}.f1.b"] = lin(f"{p}.feed_forward.intermediate_dense.weight"), f32(f"{p}.feed_forward.intermediate_dense.bias")
            w[f"{i}.f2.w"], w[f"{i}.f2.b"] = lin(f"{p}.feed_forward.output_dense.weight"), f32(f"{p}.feed_forward.output_dense.bias")
            w[f"{i}.ln2.g"], w[f"{i}.ln2.b"] = f32(f"{p}.final_layer_norm.weight"), f32(f"{p}.final_layer_norm.bias")
        return w

    # ---- forward
    @staticmethod
    def _windows(x, k, s):
        """The conv's window matrix as an overlapping row view: x (T, C) contiguous -> (T_out, k*C) with lda = s*C (no copy)."""
        T, C = x.shape
        return torch.as_strided(x, ((T - k) // s + 1, k * C), (s * C, 1))

    def _frames(self, n):
        """frames the feature encoder makes of n samples (transformers' _get_feat_extract_output_lengths); 0 once a layer runs dry"""
        for k, s in zip(self._cfg["conv_kernel"], self._cfg["conv_stride"]):
            if n < k:
                return 0
            n = (n - k) // s + 1
        return n

    def _utterance_lengths(self, input_values, attention_mask):
        """The valid sample count of every row of the batch, from the argument checks alone (no device work)."""
        if input_values.dim() != 2:
            raise ValueError("input_values must be (batch, n_samples)")
        B, n = input_values.shape
        if self._cfg["feat_extract_norm"] != "layer":
            # GroupNorm runs over time, so a padded utterance is not the utterance run alone: this family is used unmasked, one at a time
            if attention_mask is not None:
                raise NotImplementedError("attention_mask: wav2vec2-base-960h is used unmasked (its processor returns no mask; Net.py:639-644)")
            if B != 1:
                raise ValueError("input_values must be (1, n_samples): one utterance per call (Net.py:639)")
            return [n]
        if B < 1:
            raise ValueError("input_values must hold at least one utterance")
        if attention_mask is None:
            return [n] * B
        mask = torch.as_tensor(attention_mask)
        if tuple(mask.shape) != (B, n):
            raise ValueError(f"attention_mask {tuple(mask.shape)} must have input_values' shape {(B, n)}")
        mask = mask.cpu()
        if not bool(((mask == 0) | (mask == 1)).all()):
            raise ValueError("attention_mask must hold 0 / 1")
        lens = [int(v) for v in (mask != 0).sum(1)]
        for b, ln in enumerate(lens):
            if bool((mask[b, :ln] == 0).any()):
                raise ValueError(f"attention_mask row {b} is not right-padded (ones, then zeros)")
        return lens

    @torch.no_grad()
    def forward(self, input_values, attention_mask=None, conv0_route=None, **_ignored):
        """input_values (B, n) f32 [+ attention_mask (B, n) of 0 / 1, right-padded; feat_extract_norm "layer" models only] ->
        last_hidden_state (B, T_max, H) f32 with T_max = frames(n).  Utterance b runs alone on its valid prefix input_values[b, :len_b] and
        lands in rows [0, T_b), T_b = frames(len_b); rows from T_b on are ZERO.  At the valid rows that is what transformers computes for
        the padded, masked batch - no normalisation of this family runs over time, transformers zeroes the padded frames in front of the
        positional conv and masks the padded keys - while at the rows from T_b on transformers returns values that depend on the padding
        and that no caller may use."""
        route = self.conv0_route if conv0_route is None else conv0_route
        if route not in self.CONV0_ROUTES:
            raise ValueError(f"conv0_route={route!r} must be one of {self.CONV0_ROUTES}")
        lens = self._utterance_lengths(input_values, attention_mask)
        k0 = self._cfg["conv_kernel"][0]
        for ln in lens:         # every layer must keep at least one frame: refuse before the first launch, not at the layer that runs dry
            if ln < k0:
                raise ValueError("input_values shorter than the first convolution's kernel")
            if self._frames(ln) < 1:
                raise ValueError("input_values too short for the feature encoder")
        self._need()
        if len(lens) == 1 and lens[0] == input_values.shape[1]:
            return SimpleNamespace(last_hidden_state=self._encode(input_values[0], route).unsqueeze(0))
        out = torch.zeros(len(lens), self._frames(input_values.shape[1]), self._cfg["hidden_size"], device=self.device, dtype=torch.float32)
        for b, ln in enumerate(lens):
            y = self._encode(input_values[b, :ln], route)
            out[b, :y.shape[0]] = y
        return SimpleNamespace(last_hidden_state=out)

    def _feature_encoder_layer0(self, wave, route):
        """wave (n,) f32 on the device -> (T0, conv_dim[0]) rows in the compute dtype: conv 0 (+ bias), its norm, GELU"""
        c, w, dtp = self._cfg, self._w, self.dtype
        k0, s0 = c["conv_kernel"][0], c["conv_stride"][0]
        layer = c["feat_extract_norm"] == "layer"
        if layer and route == "fused" and ops.wav_conv0_ln_act_ok(wave.shape[0], c["conv_dim"][0], k0, s0):
            return ops.wav_conv0_ln_act(wave, w["conv0.f32"], w["conv0.b32"], w["cln0.g"], w["cln0.b"], s0, 1e-5, gelu=True, dtype=dtp)
        # Cin = 1: the (T0, k0) window matrix, padded to 16-byte rows (index / pad only)
        a0 = torch.nn.functional.pad(wave.unfold(0, k0, s0), (0, round_up(k0, 8) - k0)).contiguous()
        h = ops.gemm(ops.convert(a0, dtp), w["conv0"], w["conv0.b"])
        if layer:
            return ops.layer_norm_act(h, w["cln0.g"], w["cln0.b"], 1e-5, gelu=True)
        return ops.channel_norm(h, w["gn.g"], w["gn.b"], 1e-5, gelu=True)            # GroupNorm(C, C) over time, then GELU

    def _feature_encoder(self, wave, route):
        """wave (n,) f32 on the device -> (T, conv_dim[-1]) rows in the compute dtype"""
        c, w = self._cfg, self._w
        layer = c["feat_extract_norm"] == "layer"
        h = self._feature_encoder_layer0(wave, route)
        for i in range(1, len(c["conv_kernel"])):
            k, s = c["conv_kernel"][i], c["conv_stride"][i]
            if h.shape[0] < k:
                raise ValueError("input_values too short for the feature encoder")
            h = ops.gemm(self._windows(h, k, s), w[f"conv{i}"], w[f"conv{i}.b"])
            h = ops.layer_norm_act(h, w[f"cln{i}.g"], w[f"cln{i}.b"], 1e-5, gelu=True) if layer else ops.act(h, "gelu")
        return h

    def _encode(self, wave, route):
        """one utterance (n,) -> (T, H) f32"""
        c, w, dtp, dev = self._cfg, self._w, self.dtype, self.device
        eps = c["layer_norm_eps"]
        h = self._feature_encoder(wave.to(dev).float().contiguous(), route)
        T = h.shape[0]
        h = ops.gemm(ops.layer_norm(h, w["fp.ln.g"], w["fp.ln.b"], eps), w["fp.w"], w["fp.b"])          # (T, H)
        H = h.shape[1]
        # positional convolution: k = 128, pad 64, groups of H/G channels; the last output step is dropped (even kernel)
        kp, G = c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"]
        cg = H // G
        xp = torch.zeros(G, T + 2 * (kp // 2), cg, device=dev, dtype=dtp)
        xp[:, kp // 2:kp // 2 + T] = h.view(T, G, cg).permute(1, 0, 2)                                  # group-major, zero-padded in time (copy)
        pos = torch.empty(T, H, device=dev, dtype=dtp)
        n_out = T          # (an even kernel yields T + 1 steps, the last one dropped; an odd one yields T)
        for gi in range(G):
            ops.gemm(torch.as_strided(xp[gi], (n_out, kp * cg), (cg, 1)), w["pos.w"][gi], w["pos.b"][gi], out=pos[:, gi * cg:(gi + 1) * cg])
        h = ops.add(h, ops.act(pos, "gelu"))
        nh = c["num_attention_heads"]
        if c["do_stable_layer_norm"]:       # pre-LN layers, encoder.layer_norm last
            h = run_clip_layers(h, w["layers"], n_layers=c["num_hidden_layers"], B=1, L=T, H=H, heads=nh, eps=eps, act="gelu", causal=False)
            return ops.convert(ops.layer_norm(h, w["enc.ln.g"], w["enc.ln.b"], eps), torch.float32)
        h = ops.layer_norm(h, w["enc.ln.g"], w["enc.ln.b"], eps)
        d = H // nh
        for i in range(c["num_hidden_layers"]):
            qk = ops.gemm(h, w[f"{i}.qk.w"], w[f"{i}.qk.b"])
            vt = ops.gemm(h, w[f"{i}.v.w"], w[f"{i}.v.b"], transpose_rows=T, transpose_ld=round_up(T, 8))
            att = ops.attention(qk[:, :H], qk[:, H:], vt, T, B=1, Lq=T, heads=nh, d=d, scale=d ** -0.5)
            h = ops.layer_norm(ops.gemm(att, w[f"{i}.o.w"], w[f"{i}.o.b"], residual=h), w[f"{i}.ln1.g"], w[f"{i}.ln1.b"], eps)
            f = ops.act(ops.gemm(h, w[f"{i}.f1.w"], w[f"{i}.f1.b"]), "gelu")
            h = ops.layer_norm(ops.gemm(f, w[f"{i}.f2.w"], w[f"{i}.f2.b"], residual=h), w[f"{i}.ln2.g"], w[f"{i}.ln2.b"], eps)
        return ops.convert(h, torch.float32)


def normalize_waveform(x: torch.Tensor) -> torch.Tensor:
    """What `self.processor(waveform, sampling_rate=..., return_tensors='pt').input_values` does for wav2vec2-base-960h (Net.py:639;
    Wav2Vec2FeatureExtractor do_normalize=True): zero mean, unit variance per utterance, (x - mean) / sqrt(var + 1e-7).  Host-side
    input preparation, like the processor's numpy code."""
    x = x.float().reshape(1, -1)
    return (x - x.mean(-1, keepdim=True)) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + 1e-7)


class Wav2VecFeatureExtractor:
    """Net.py:607-667: `model` is a Wav2Vec2Model with caller-loaded weights (the reference downloads 'facebook/wav2vec2-base-960h').
    `extract_features(waveform)` takes the mono 16 kHz samples `sf.read` / `librosa.resample` produce (Net.py:627-636) and returns what
    extract_features_from_wav returns: (T, (m + n + 1) * hidden) f32.  With `sample_rate=` the samples are at that rate and the whole
    signal path runs on the device (emote_hack_amd.audio_io.prepare_waveform: downmix + resampling + normalisation kernels);
    `extract_features_from_wav` also takes the file's path, like the reference."""
    sampling_rate = 16000

    def __init__(self, model: Wav2Vec2Model, device="cuda"):
        self.model, self.device = model, torch.device(device)

    def extract_features(self, waveform, m: int = 2, n: int = 2, sample_rate=None) -> torch.Tensor:
        from .conditioning import audio_windows
        if sample_rate is not None:        # any rate (16000 too): the device front-end
            from .audio_io import prepare_waveform
            return audio_windows(self.model(prepare_waveform(waveform, sample_rate, self.device)).last_hidden_state, m, n)
        wf = torch.as_tensor(waveform, dtype=torch.float32)
        if wf.dim() > 1:
            wf = wf.mean(dim=1)                                    # multi-channel audio: mean over channels (Net.py:634-636)
        hs = self.model(normalize_waveform(wf).to(self.device)).last_hidden_state
        return audio_windows(hs, m, n)

    def extract_features_from_wav(self, audio, m: int = 2, n: int = 2, sample_rate=None) -> torch.Tensor:
        """Net.py:614-667: `audio` is the path of a .wav file (read by emote_hack_amd.audio_io.read_wav, at the file's own rate), or
        the samples themselves as in extract_features."""
        if isinstance(audio, (str, os.PathLike)):
            from .audio_io import read_wav
            audio, sample_rate = read_wav(audio)
        return self.extract_features(audio, m, n, sample_rate)

    def extract_features_from_mp4(self, video_path, m: int = 2, n: int = 2) -> torch.Tensor:
        """Net.py:670-735 reads `<video>.wav` beside the video and writes it from the container first when it is missing (:683-692).
        Demuxing is not built here: without that .wav this is a ValueError."""
        audio_path = os.path.splitext(os.fspath(video_path))[0] + ".wav"
        if not os.path.exists(audio_path):
            raise ValueError(f"extract_features_from_mp4: {audio_path!r} does not exist and demuxing a video container is not built - "
                             "extract the audio track to that .wav first (e.g. ffmpeg -i video.mp4 video.wav), or pass the samples")
        return self.extract_features_from_wav(audio_path, m, n)
