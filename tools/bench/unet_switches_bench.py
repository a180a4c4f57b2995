"""What the two off-config UNet switches cost (profiles/unet_switches.md):

  (1) the modulated GroupNorm (ops.group_norm(mod=): emo_groupnorm_apply_mod / emo_groupnorm_mod) against the plain one at the three
      joint-norm shapes of the cfg2 step, bf16, HIP events around a graph of 20 launches each, plain and modulated alternating;
  (2) one forward of the SD-1.5-size backbone (cfg2 geometry: [uncond, cond] x 12 frames x 64x64 latents, bf16) with neither switch,
      unet_use_temporal_attention=True, resnet_time_scale_shift="scale_shift", and both - HIP events around eager launches.

    python tools/bench/unet_switches_bench.py [--skip-model]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from emote_hack_amd import ops as o  # noqa: E402

DEV, DT = "cuda", torch.bfloat16


def clocks():
    """shader / memory clock (MHz) as bench.py reads them (amdgpu sysfs tables); None where the node is not readable"""
    import bench
    return bench.gpu_clocks(0)


def graph_of(f, n=20):
    for _ in range(3):
        f()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        f()
        with torch.cuda.graph(g, stream=s):
            for _ in range(n):
                f()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    return g, n


def time_graph(gn, reps=5):
    g, n = gn
    best = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best.append(e0.elapsed_time(e1) / n * 1e3)
    return best


def groupnorm_table():
    rows = []
    for N, S, C in ((2, 12 * 64 * 64, 320), (2, 12 * 32 * 32, 640), (2, 12 * 8 * 8, 1280)):
        x = torch.randn(N * S, C, device=DEV).to(DT)
        gamma, beta = 1 + 0.1 * torch.randn(C, device=DEV), 0.1 * torch.randn(C, device=DEV)
        mod = torch.cat([0.5 * torch.randn(N, C, device=DEV), torch.randn(N, C, device=DEV)], 1).contiguous()
        y = torch.empty_like(x)
        plain = graph_of(lambda: o.group_norm(x, gamma, beta, N, 32, 1e-5, True, out=y))
        modul = graph_of(lambda: o.group_norm(x, gamma, beta, N, 32, 1e-5, True, out=y, mod=mod))
        tp, tm = [], []
        for _ in range(4):      # alternate the two: drift hits both alike
            tp += time_graph(plain)
            tm += time_graph(modul)
        med = lambda v: sorted(v)[len(v) // 2]
        rows.append(dict(N=N, S=S, C=C, plain_us=med(tp), plain_min=min(tp), plain_max=max(tp), mod_us=med(tm), mod_min=min(tm), mod_max=max(tm),
                         bytes=2 * 2 * N * S * C, extra_bytes=4 * N * 2 * C))
        r = rows[-1]
        print(f"GN N={N} S={S:6d} C={C:5d}: plain {r['plain_us']:7.2f} us [{r['plain_min']:.2f}, {r['plain_max']:.2f}]   mod {r['mod_us']:7.2f} us "
              f"[{r['mod_min']:.2f}, {r['mod_max']:.2f}]   ratio {r['mod_us'] / r['plain_us']:.3f}", flush=True)
    return rows


def model_table():
    from emote_hack_amd.spec import param_shapes
    from emote_hack_amd.synth import seeded_randn, synth_state_dict
    from emote_hack_amd.unet import UNet3DConditionModel
    from tests import cases
    x, ctx = seeded_randn((2, 4, 12, 64, 64), 1).to(DEV), seeded_randn((2, 77, 768), 2).to(DEV)
    rows = []
    for name, extra in (("neither", {}), ("unet_use_temporal_attention", dict(unet_use_temporal_attention=True)),
                        ("resnet_time_scale_shift", dict(resnet_time_scale_shift="scale_shift")),
                        ("both", dict(unet_use_temporal_attention=True, resnet_time_scale_shift="scale_shift"))):
        m = UNet3DConditionModel(**dict(cases.SD15_MOTION, **extra))
        m.load_state_dict(synth_state_dict(param_shapes(m.spec), device=DEV))
        m.to(DEV, DT)
        for _ in range(3):
            m(x, 981, ctx, _return_rows=True)
        torch.cuda.synchronize()
        ts = []
        for _ in range(10):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            m(x, 981, ctx, _return_rows=True)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        rows.append(dict(name=name, ms=sorted(ts)[len(ts) // 2], ms_min=min(ts), ms_max=max(ts)))
        print(f"forward cfg2 geometry, {name}: {rows[-1]['ms']:.2f} ms [{min(ts):.2f}, {max(ts):.2f}]", flush=True)
        del m
        torch.cuda.empty_cache()
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=None, help="write the tables as JSON here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = dict(device=torch.cuda.get_device_name(0), clocks_before=clocks())
    res["groupnorm"] = groupnorm_table()
    if not a.skip_model:
        res["forward"] = model_table()
    res["clocks_after"] = clocks()
    print(json.dumps(res["clocks_after"]))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)
