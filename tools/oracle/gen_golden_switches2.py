#!/usr/bin/env python3
"""Generate tests/golden/unet_switches2.{safetensors,json} by running the REFERENCE's own in-tree code (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/oracle/gen_golden_switches2.py

The two UNet3DConditionModel ctor switches no shipped config turns on: `unet_use_temporal_attention=True` (the attn_temp branch of
BasicTransformerBlock, attention.py:235-246,309-318; mutual_self_attention.py:274-282) and `resnet_time_scale_shift="scale_shift"`
(resnet.py:149-156,188-195).  Same shim and load_synth pattern as gen_golden.py (imported for its helpers; none of its outputs is
rewritten): the reference modules carry name-keyed synthetic weights - `attn_temp.to_out[0].weight` is zero-initialised by the ctor
(attention.py:245), which would make the branch an identity; load_synth overwrites it - and ONLY tensors / key listings are stored.
"""
from __future__ import annotations

import copy
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import gen_golden as gg  # noqa: E402  (installs the shim, imports the reference modules)
import torch  # noqa: E402
from safetensors.torch import save_file  # noqa: E402

from emote_hack_amd.synth import seeded_randn  # noqa: E402
from tests import cases  # noqa: E402

TEMP = dict(unet_use_temporal_attention=True)
SS = dict(resnet_time_scale_shift="scale_shift")
T_STEP = 961


def lowp(T, name, fn):
    """the reference's OWN bf16 / fp16 forward of the same model and inputs (the yard-stick of the low-precision HIP modes)"""
    for tag, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        T[f"{name}_{tag}"] = fn(dt).float()


def main():
    T, J = {}, {}
    x, ctx = cases.tiny_inputs(2, 4)
    models = {}
    for name, base, extra in (("temp", cases.TINY_MOTION, TEMP), ("ss", cases.TINY_MOTION, SS), ("both", cases.TINY_MOTION, dict(TEMP, **SS)),
                              ("both_linear", cases.TINY_LINEAR, dict(TEMP, **SS))):
        u = gg.load_synth(gg.UNet3DConditionModel(**dict(base, **extra)))
        models[name] = u
        T[f"{name}/out"] = u(x, T_STEP, ctx).sample
        lowp(T, f"{name}/out", lambda dt, u=u: copy.deepcopy(u).to(dt)(x.to(dt), T_STEP, ctx.to(dt)).sample)
        assert bool(torch.isfinite(T[f"{name}/out"]).all())
    J["both_keys"] = gg.key_listing(models["both"])
    J["both_linear_keys"] = gg.key_listing(models["both_linear"])
    # the switches are live
    plain = gg.load_synth(gg.UNet3DConditionModel(**cases.TINY_MOTION))(x, T_STEP, ctx).sample
    J["max_abs_diff_vs_unswitched"] = {k: float((T[f"{k}/out"] - plain).abs().max()) for k in ("temp", "ss", "both")}
    assert all(v > 1e-2 for v in J["max_abs_diff_vs_unswitched"].values()), J["max_abs_diff_vs_unswitched"]
    # ReferenceNet write -> fp16 banks -> read with CFG batch 2, on the model with attn_temp (mutual_self_attention.py:274-282)
    ref = gg.load_synth(gg.UNet3DConditionModel(**cases.TINY), cases.REF_PREFIX)
    banks = gg.run_writer(ref, seeded_randn((1, 4, 16, 16), 3).repeat(2, 1, 1, 1), T_STEP, ctx)
    u = models["temp"]
    T["temp/read_out"] = gg.run_reader(u, x, T_STEP, ctx, banks)
    lowp(T, "temp/read_out", lambda dt: gg.run_reader(copy.deepcopy(u).to(dt), x.to(dt), T_STEP, ctx.to(dt), [b.to(dt) for b in banks],
                                                      bank_dtype=None if dt == torch.float16 else dt))
    # module level: the reference classes alone
    for name, cin, cout in (("resnet_ss_sc", 32, 64), ("resnet_ss_id", 64, 64)):
        m = gg.load_synth(gg.ref_resnet.ResnetBlock3D(in_channels=cin, out_channels=cout, temb_channels=128, groups=8, eps=1e-5,
                                                      non_linearity="silu", time_embedding_norm="scale_shift"), name + ".")
        T[f"{name}/out"] = m(seeded_randn((2, cin, 3, 8, 8), 211), seeded_randn((2, 128), 212))
    m = gg.load_synth(gg.ref_attention.BasicTransformerBlock(64, 4, 16, cross_attention_dim=32, unet_use_cross_frame_attention=False,
                                                             unet_use_temporal_attention=True), "btb_temp.")
    T["btb_temp/out"] = m(seeded_randn((2 * 4, 16, 64), 213), encoder_hidden_states=seeded_randn((2 * 4, 5, 32), 214), video_length=4)
    save_file({k: v.contiguous() for k, v in T.items()}, os.path.join(gg.GOLD, "unet_switches2.safetensors"))
    json.dump(J, open(os.path.join(gg.GOLD, "unet_switches2.json"), "w"), indent=0, sort_keys=True)
    print("unet_switches2.safetensors", {k: tuple(v.shape) for k, v in T.items()})
    print("unet_switches2.json", {k: (len(v) if isinstance(v, dict) else v) for k, v in J.items()}, J["max_abs_diff_vs_unswitched"])


if __name__ == "__main__":
    main()
