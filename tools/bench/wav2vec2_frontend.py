#!/usr/bin/env python3
"""Time the feature encoder of the wav2vec2-large family (LARGE_CONFIG: a LayerNorm + GELU behind every conv) in bf16 on 10 s and 60 s
of 16 kHz audio, synthetic name-keyed weights:

  layer0     conv 0 + LayerNorm + GELU by emo_wav_conv0_ln_act ("fused") against the window matrix (unfold + pad + contiguous +
             convert) + K = 16 GEMM + emo_layernorm_act ("gemm") - the two `conv0_route`s of Wav2Vec2Model
  layers1-6  row-view GEMM + bias, then emo_layernorm_act ("ln_act") against emo_layernorm + emo_act ("ln+act")
  forward    the whole 24-layer forward on both routes

The variants of a comparison alternate inside one loop; every call is bracketed by device events on the launch stream and the median,
min and max over --iters calls after --warmup are reported, with the bytes each layer-0 route moves by its tensor sizes (arithmetic,
not a counter).

    timeout -k 10 600 python tools/bench/wav2vec2_frontend.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402


def timed(variants, iters, warmup):
    """variants {name: fn} -> {name: {median, min, max} ms}; the variants alternate call by call"""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(iters):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seconds", type=int, nargs="+", default=[10, 60])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from emote_hack_amd import ops
    from emote_hack_amd.wav2vec2 import LARGE_CONFIG, Wav2Vec2Model, normalize_waveform, wav2vec2_synth_state_dict
    dtp = torch.bfloat16
    m = Wav2Vec2Model(LARGE_CONFIG)
    m.load_state_dict(wav2vec2_synth_state_dict(LARGE_CONFIG, device="cuda"))          # device draws: 315 M parameters
    m.to("cuda", dtp)
    c, w = m._cfg, m._w
    res = {"what": "wav2vec2-large feature encoder and forward, bf16, synthetic weights", "device": torch.cuda.get_device_name(0),
           "iters": a.iters, "warmup": a.warmup, "runs": {}}
    for secs in a.seconds:
        n = 16000 * secs
        x = normalize_waveform(torch.randn(n, generator=torch.Generator().manual_seed(secs))).to("cuda")
        wave = x[0].contiguous()
        k0, s0, C0 = c["conv_kernel"][0], c["conv_stride"][0], c["conv_dim"][0]
        T0 = (n - k0) // s0 + 1
        r = {"samples": n, "rows_layer0": T0}
        r["layer0_ms"] = timed({"fused": lambda: m._feature_encoder_layer0(wave, "fused"), "gemm": lambda: m._feature_encoder_layer0(wave, "gemm")},
                               a.iters, a.warmup)
        kp = (k0 + 7) // 8 * 8
        # by tensor sizes: fused = waveform in, rows out; gemm = waveform in, f32 window matrix out and in, bf16 copy out and in, pre-norm
        # rows out and in, rows out
        r["layer0_bytes_by_tensor_sizes"] = {"fused": 4 * n + 2 * T0 * C0,
                                             "gemm": 4 * n + 2 * 4 * T0 * kp + 2 * 2 * T0 * kp + 3 * 2 * T0 * C0}
        h0 = m._feature_encoder_layer0(wave, "fused")

        def rest(fused_act):
            h = h0
            for i in range(1, len(c["conv_kernel"])):
                h = ops.gemm(m._windows(h, c["conv_kernel"][i], c["conv_stride"][i]), w[f"conv{i}"], w[f"conv{i}.b"])
                if fused_act:
                    h = ops.layer_norm_act(h, w[f"cln{i}.g"], w[f"cln{i}.b"], 1e-5, gelu=True)
                else:
                    h = ops.act(ops.layer_norm(h, w[f"cln{i}.g"], w[f"cln{i}.b"], 1e-5), "gelu")
            return h

        r["layers1_6_ms"] = timed({"ln_act": lambda: rest(True), "ln+act": lambda: rest(False)}, a.iters, a.warmup)
        r["forward_ms"] = timed({"fused": lambda: m(x, conv0_route="fused"), "gemm": lambda: m(x, conv0_route="gemm")}, max(a.iters // 3, 3), 2)
        y = m(x).last_hidden_state
        assert y.shape == (1, m._frames(n), 1024) and bool(torch.isfinite(y).all())
        r["frames"] = y.shape[1]
        res["runs"][f"{secs}s"] = r
        print(json.dumps({f"{secs}s": r}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
