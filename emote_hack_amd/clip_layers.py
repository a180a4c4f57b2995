"""What CLIP's text and vision towers share (transformers' CLIPEncoder): the per-layer keys, their packing, the pre-LN layer loop and
the local-checkpoint reader.

  layer        pre-LN: LN1 folded into the q | k projection and into the V^T projection (two launches: the split V^T store of one launch
               needs M % 32 == 0, and neither 2 x 77 nor 257 rows are), emo_attention, out_proj + residual, LN2 folded into fc1, emo_act,
               fc2 + residual
"""
from __future__ import annotations

import json
import os

import torch

from . import ops
from .module import ln_fold_weights, round_up

ACTS = {"quick_gelu": "quick_gelu", "gelu": "gelu"}


def clip_layer_shapes(prefix, n_layers, H, I):
    """keys / shapes of `<prefix>.<i>.*`, transformers' CLIPEncoderLayer names, in registration order"""
    d = {}
    for i in range(n_layers):
        p = f"{prefix}.{i}"
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
    return d


def pack_clip_layers(sd, prefix, n_layers, dev, dtp):
    """-> {"<i>.qk", "<i>.v", "<i>.f1": (W * gamma, its row sums, b + W . beta), "<i>.o.w", "<i>.o.b", "<i>.f2.w", "<i>.f2.b"} on `dev`;
    sd holds host f32 masters, every product is formed on the device."""
    f32 = lambda k: sd[k].to(dev).float().contiguous()
    lin = lambda k: sd[k].to(dev, dtp).contiguous()

    def fold(wt, b, norm):
        return ln_fold_weights(wt.to(dev), b.to(dev), sd[norm + ".weight"].to(dev), sd[norm + ".bias"].to(dev), dtp)

    w = {}
    for i in range(n_layers):
        ly = f"{prefix}.{i}"
        p, m = f"{ly}.self_attn", f"{ly}.mlp"
        w[f"{i}.qk"] = fold(torch.cat([sd[f"{p}.q_proj.weight"], sd[f"{p}.k_proj.weight"]]),
                            torch.cat([sd[f"{p}.q_proj.bias"], sd[f"{p}.k_proj.bias"]]), f"{ly}.layer_norm1")
        w[f"{i}.v"] = fold(sd[f"{p}.v_proj.weight"], sd[f"{p}.v_proj.bias"], f"{ly}.layer_norm1")
        w[f"{i}.o.w"], w[f"{i}.o.b"] = lin(f"{p}.out_proj.weight"), f32(f"{p}.out_proj.bias")
        w[f"{i}.f1"] = fold(sd[f"{m}.fc1.weight"], sd[f"{m}.fc1.bias"], f"{ly}.layer_norm2")
        w[f"{i}.f2.w"], w[f"{i}.f2.b"] = lin(f"{m}.fc2.weight"), f32(f"{m}.fc2.bias")
    return w


def run_clip_layers(h, w, *, n_layers, B, L, H, heads, eps, act, causal, collect=None):
    """h (B * L, H) rows through the layers packed in `w`; appends every layer's output to `collect` when given."""
    d = H // heads
    for i in range(n_layers):
        st = ops.layer_norm_stats(h, eps)
        wq, cs, bq = w[f"{i}.qk"]
        qk = ops.gemm(h, wq, bq, ln=(cs, st))                                                 # LN1 -> q | k
        wv, cs, bv = w[f"{i}.v"]
        vt = ops.gemm(h, wv, bv, ln=(cs, st), transpose_rows=L, transpose_ld=round_up(L, 8))  # LN1 -> V^T (B, H, ld)
        att = ops.attention(qk[:, :H], qk[:, H:], vt, L, B=B, Lq=L, heads=heads, d=d, scale=d ** -0.5, causal=causal)
        h = ops.gemm(att, w[f"{i}.o.w"], w[f"{i}.o.b"], residual=h)
        st = ops.layer_norm_stats(h, eps)
        w1, cs, b1 = w[f"{i}.f1"]
        f = ops.act(ops.gemm(h, w1, b1, ln=(cs, st)), act)                                    # LN2 -> fc1 -> activation
        h = ops.gemm(f, w[f"{i}.f2.w"], w[f"{i}.f2.b"], residual=h)
        if collect is not None:
            collect.append(h)
    return h


def load_local_checkpoint(pretrained_model_path, subfolder):
    """A LOCAL checkpoint folder (`<path>/<subfolder>/config.json` + `model.safetensors` or `pytorch_model.bin`) -> (config dict,
    state dict) - nothing is fetched."""
    path = os.path.join(pretrained_model_path, subfolder) if subfolder else pretrained_model_path
    config_file = os.path.join(path, "config.json")
    if not os.path.isfile(config_file):
        raise RuntimeError(f"{config_file} does not exist")
    with open(config_file) as f:
        config = json.load(f)
    st_file, bin_file = os.path.join(path, "model.safetensors"), os.path.join(path, "pytorch_model.bin")
    if os.path.isfile(st_file):
        from safetensors.torch import load_file
        return config, load_file(st_file)
    if os.path.isfile(bin_file):
        return config, torch.load(bin_file, map_location="cpu", weights_only=True)
    raise RuntimeError(f"neither {st_file} nor {bin_file} exists")
