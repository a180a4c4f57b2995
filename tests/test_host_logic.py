"""CPU tests of host-side logic that needs no device: the GEMM planner's split-K rules through the C ABI (pure host code in
libemo_hip.so) and the algebra of the two linear-map compositions the UNet packs at load time."""
import os

import pytest
import torch

from emote_hack_amd import _lib
from emote_hack_amd.synth import seeded_randn
from tests import cases

BF16, F32 = 1, 0


def _dt(name):
    from emote_hack_amd import ops
    return ops.dt(torch.zeros(1, dtype=name))


def test_planner_split_k_rules():
    """emo_gemm_suggest_split_k (csrc/gemm_api.h plan_gemm): the measured rules of DESIGN.md section 7."""
    lib = _lib.load()
    bf16, f32 = _dt(torch.bfloat16), _dt(torch.float32)
    sk = lambda M, N, K, dt=bf16, geglu=0, tr=0: lib.emo_gemm_suggest_split_k(M, N, K, dt, geglu, tr)
    # the 8x8-level 3x3 convs (M = 1536, K = 9 * 1280 / 9 * 2560): 30 tiles of 256x256, one block per CU -> 8 ways
    assert sk(1536, 1280, 11520) == 8
    assert sk(1536, 1280, 23040) == 8
    assert sk(640, 1280, 11520) == 17          # the ReferenceNet group (T = 10): 15 tiles -> 256 // 15 slices
    # f32 (validation mode) keeps the 128x128 tiles split to fill 512 slots
    assert sk(1536, 1280, 11520, f32) == 4
    # big single-pass shapes never split; short-K few-block shapes take 64x64 tiles unsplit (K = 2560 included)
    assert sk(98304, 2560, 320, geglu=1) == 1
    assert sk(1536, 1280, 1280) == 1
    assert sk(1536, 1280, 2560) == 1
    # long-K dense with few 128-row blocks still splits (ff.net.2 + proj_out tail of the 8x8 level: K = 6400)
    assert sk(1536, 1280, 6400) > 1
    # the workspace the caller must supply
    assert lib.emo_gemm_workspace_bytes(1536, 1280, 8) == 8 * 1536 * 1280 * 4
    assert lib.emo_gemm_workspace_bytes(1536, 1280, 1) == 0


def test_ff_tail_weights_compose_the_two_linears():
    """unet.ff_tail_weights: (g W2^T + b2 + h) Wo^T + bo == [g | h] Wt^T + bt, for a Linear and for a 1x1-conv proj_out."""
    from emote_hack_amd.unet import ff_tail_weights
    C, M = 24, 50
    g, h = seeded_randn((M, 4 * C), 1).double(), seeded_randn((M, C), 2).double()
    w2, b2 = seeded_randn((C, 4 * C), 3), seeded_randn((C,), 4)
    wo, bo = seeded_randn((C, C), 5), seeded_randn((C,), 6)
    ref = (g @ w2.double().t() + b2.double() + h) @ wo.double().t() + bo.double()
    for w_out in (wo, wo.reshape(C, C, 1, 1)):
        wt, bt = ff_tail_weights(w_out, bo, w2, b2)
        assert tuple(wt.shape) == (C, 5 * C) and tuple(bt.shape) == (C,) and wt.dtype == torch.float32
        got = torch.cat([g, h], 1) @ wt.double().t() + bt.double()
        torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-5)


def test_groupnorm_fold_algebra():
    """What emo_groupnorm_fold_linear builds (emo_hip.h): GN(x) W^T + b == x W'_n^T + b'_n per instance, with
    W'_n = W diag(gamma * rstd_n), b'_n = b + W beta - sum_c mean_n[c] W'_n[:, c] - restated in torch f64 against
    group_norm -> linear (the GPU test holds the kernel to the same statement)."""
    import torch.nn.functional as F
    N, S, C, G, Co = 3, 40, 32, 8, 12
    x = (seeded_randn((N, S, C), 7) * 1.7 + 0.4).double()
    gamma, beta = (1 + 0.1 * seeded_randn((C,), 8)).double(), (0.1 * seeded_randn((C,), 9)).double()
    w, b = seeded_randn((Co, C), 10).double(), seeded_randn((Co,), 11).double()
    ref = F.linear(F.group_norm(x.permute(0, 2, 1), G, gamma, beta, 1e-6).permute(0, 2, 1), w, b)
    xg = x.reshape(N, S, G, C // G)
    mean = xg.mean((1, 3))                                              # (N, G)
    rstd = (xg.var((1, 3), unbiased=False) + 1e-6).rsqrt()
    mean_c, rstd_c = mean.repeat_interleave(C // G, 1), rstd.repeat_interleave(C // G, 1)   # (N, C)
    wn = w[None] * (gamma[None] * rstd_c)[:, None, :]                   # (N, Co, C)
    bn = b[None] + (w @ beta)[None] - torch.einsum("nc,noc->no", mean_c, wn)
    got = torch.einsum("nsc,noc->nso", x, wn) + bn[:, None, :]
    torch.testing.assert_close(got, ref, rtol=1e-9, atol=1e-9)


def test_reference_group_size_never_exceeds_the_step_count():
    """ReferenceNet timesteps per batched pass (pipeline.reference_group_size): 1 <= T <= n_steps always; on several ranks a
    multiple of the world size whenever the step count allows it (10 over 8 ranks -> 16, never 16 of a 12-step loop), so no
    rank computes a padded timestep; and the groups tile the loop exactly."""
    from emote_hack_amd.pipeline import EMOAnimationPipeline as P
    for n_steps in (1, 2, 3, 7, 12, 20, 25, 50, 1000):
        for world in (1, 2, 3, 4, 8, 16):
            for want in (0, 1, 2, 5, 10, 25, 50, 10**6):
                T = P.reference_group_size(want, n_steps, world)
                assert 1 <= T <= n_steps, (want, n_steps, world, T)
                if world > 1 and T < n_steps:
                    assert T % world == 0, (want, n_steps, world, T)
                groups = [list(range(i, min(i + T, n_steps))) for i in range(0, n_steps, T)]
                assert sum(len(g) for g in groups) == n_steps and all(len(g) <= T for g in groups)
    assert P.reference_group_size(10, 50, 8) == 16 and P.reference_group_size(10, 12, 8) == 12 and P.reference_group_size(10, 50, 1) == 10


def test_strong_mode_deals_one_unit_per_rank_at_eight_gpus():
    """bench.py --mode strong = BASELINE configs[3]: one 48-frame clip = 4 windows x 2 CFG branches = 8 units; U[r::8] hands every
    rank exactly one, U[r::4] a [uncond, cond] pair of ONE window (shared prefix), U[r::2] two such pairs."""
    from emote_hack_amd.denoise_loop import loop_plan
    plan = lambda world, r: loop_plan(48, 50, 50, context_frames=12, context_stride=1, context_overlap=0, dist=world > 1, rank=r, world_size=world)
    units = plan(1, 0).units
    assert len(units) == 8 and all(plan(8, r).units == units for r in range(8))
    assert all(len(units[r::8]) == 1 for r in range(8))
    assert all([c.units for c in plan(8, r).calls] == [units[r::8]] for r in range(8))
    for world in (4, 2, 1):
        for r in range(world):
            mine = units[r::world]
            byw = {}
            for w, br in mine:
                byw.setdefault(w, set()).add(br)
            assert all(v == {0, 1} for v in byw.values()), (world, r, mine)
            calls = plan(world, r).calls
            assert sorted(u for c in calls for u in c.units) == sorted(mine)
            assert all(c.units == [(c.units[0][0], 0), (c.units[0][0], 1)] and c.halves_identical for c in calls), (world, r)


def test_groupnorm_one_launch_plan():
    """emo_groupnorm_one_launch_ok (csrc/norm.hip gn1_geom): one workgroup per (instance, slab of whole groups) only where the slab
    fits <= 32 K elements, the launch has >= 32 workgroups and a slab's channels fill whole 16-byte vectors."""
    lib = _lib.load()
    bf16, f16, f32 = _dt(torch.bfloat16), _dt(torch.float16), _dt(torch.float32)
    ok = lib.emo_groupnorm_one_launch_ok
    # the bench's norms (N instances of S rows, C channels, 32 groups): 8x8 level joint, 16x16 per frame -> one launch
    assert ok(2, 12 * 64, 1280, 32, bf16) == 1 and ok(24, 256, 1280, 32, bf16) == 1 and ok(24, 64, 1280, 32, f16) == 1
    # larger instances keep the two coalesced passes: 16x16 joint, 32x32 per frame / joint, 64x64
    assert ok(2, 12 * 256, 1280, 32, bf16) == 0 and ok(24, 1024, 640, 32, bf16) == 0 and ok(2, 12 * 4096, 320, 32, bf16) == 0
    # too few workgroups (2 instances x 8 slabs of 4 groups at 10 channels per group)
    assert ok(2, 256, 320, 32, bf16) == 0 and ok(5, 37, 320, 32, bf16) == 1
    # f32: 4-wide vectors, slabs of 2 groups at 10 channels per group
    assert ok(5, 37, 320, 32, f32) == 1
    # outside the kernels' limits (groups, width, divisibility, dtype): never
    assert ok(4, 64, 1280, 256, bf16) == 0 and ok(4, 64, 1284, 32, bf16) == 0 and ok(4, 64, 1280, 32, 7) == 0 and ok(0, 64, 1280, 32, bf16) == 0


def test_geglu_polynomial_constants():
    """The erf-GELU polynomial of the bf16 GEGLU epilogue (csrc/common.h geglu_poly2), restated in numpy f32 with the constants read
    from the header: |gelu error| <= 1.9e-4 over the fitted range, x * P(x^2) >= 0.5 from |x| = 4 on (so the output clamp alone
    makes the tails exact - the kernel has no input clamp), monotone there, and no NaN up to overflow."""
    import os
    import re
    import math
    import numpy as np
    src = open(os.path.join(os.path.dirname(_lib.HERE), "emote_hack_amd", "csrc", "common.h")).read()
    body = src[src.index("void geglu_poly2("):]
    body = body[:body.index("oa = o.x")]
    coef = [float(m) for m in re.findall(r"v2f_t\{(-?[0-9.]+e[-+]?[0-9]+)f,", body)]
    lead = float(re.search(r"v2f_t p = \{([0-9.e+-]+)f,", body).group(1))
    coef = [lead] + coef
    assert len(coef) == 7, coef

    def E(t):
        t = t.astype(np.float32)
        u = t * t
        p = np.full_like(t, np.float32(coef[0]))
        for c in coef[1:]:
            p = p * u + np.float32(c)
        return t * p

    x = np.linspace(-6, 6, 240001, dtype=np.float32)
    g = x * (np.float32(0.5) + np.clip(E(x), -0.5, 0.5))
    ref = np.array([0.5 * v * (1.0 + math.erf(v / math.sqrt(2.0))) for v in x.astype(np.float64)])
    assert np.abs(g - ref).max() <= 1.9e-4
    t = np.logspace(math.log10(4.0), 19, 200001).astype(np.float32)
    with np.errstate(over="ignore"):
        e = E(t)
    assert not np.isnan(e).any() and e.min() >= 0.5 and (np.diff(e[np.isfinite(e)]) >= 0).all()


def test_context_windows_equal_the_oracle_over_a_sweep():
    """emote_hack_amd.context.uniform (an independent restatement: integer bit reversal, explicit start / hop walk) against
    oracle.scheduler_ref.uniform_windows (the reference's formulation, pinned by tests/golden/ints.json) over a sweep of geometries,
    `step` values (the pattern rotation) and both loop modes."""
    from emote_hack_amd.context import ordered_halving, uniform
    from oracle.scheduler_ref import ordered_halving as oh_ref, uniform_windows
    for v in (0, 1, 2, 3, 5, 8, 49, 1 << 40, (1 << 64) - 1):
        assert ordered_halving(v) == oh_ref(v)
    n_cases = 0
    for step in (0, 1, 2, 3, 7, 13):
        for n in (8, 12, 17, 24, 40, 48, 96):
            for size in (4, 12, 16):
                for stride in (1, 2, 3):
                    for ov in (0, 2, 4):
                        if ov >= size:
                            continue
                        for closed in (True, False):
                            got = list(uniform(step, 50, n, size, stride, ov, closed))
                            assert got == uniform_windows(step, 50, n, size, stride, ov, closed), (step, n, size, stride, ov, closed)
                            n_cases += 1
    assert n_cases > 1000


def test_pipeline_helper_methods_equal_the_reference_method_bodies():
    """The methods of EMOAnimationPipeline around __call__ (EMOAnimationPipeline.py:341-540) against goldens produced by running the
    reference's own method bodies on stub objects (tools/oracle/gen_golden.py gen_pipeline_methods): prepare_latents (host RNG, tiled
    clip noise), prepare_condition, next_step (DDIM inversion step), interpolate_latents with slerp / linear, select_controlnet_res_samples."""
    import numpy as np
    from safetensors.torch import load_file
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd import pipeline as P
    from emote_hack_amd.synth import seeded_randn
    g = load_file(os.path.join(cases.GOLDEN_DIR, "pipeline_methods.safetensors"))
    sch = DDIMScheduler()
    pipe = P.EMOAnimationPipeline(unet=type("U", (), {"device": torch.device("cpu")})(), scheduler=sch)
    sch.set_timesteps(50)
    x, eps = seeded_randn((4, 4, 16, 16), 500), seeded_randn((4, 4, 16, 16), 501)
    for t in (1, 21, 481, 981):
        xn, x0 = pipe.next_step(eps, t, x)
        torch.testing.assert_close(xn, g[f"next_step/{t}/x_next"], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(x0, g[f"next_step/{t}/pred_x0"], rtol=1e-5, atol=1e-5)
    lat = pipe.prepare_latents(1, 4, 32, 64, 64, torch.float32, torch.device("cpu"), torch.Generator().manual_seed(5))
    assert torch.equal(lat, g["prepare_latents/out"])                      # the same host RNG stream, tiled the same way
    with pytest.raises(ValueError, match="Unexpected latents shape"):
        pipe.prepare_latents(1, 4, 32, 64, 64, torch.float32, "cpu", None, latents=torch.zeros(1, 4, 32, 8, 8))
    cond = pipe.prepare_condition(g["prepare_condition/in"].numpy(), 1, "cpu", torch.float32, True)
    assert torch.equal(cond, g["prepare_condition/out"])
    l3 = seeded_randn((1, 4, 3, 4, 4), 502)
    assert pipe.interpolate_latents(l3, 1, "cpu") is l3                      # the factor __call__ hard-codes (:824)
    for name, is_slerp in (("slerp", True), ("linear", False)):
        P.set_tensor_interpolation_method(is_slerp)
        torch.testing.assert_close(pipe.interpolate_latents(l3, 3, "cpu"), g[f"interpolate/{name}"], rtol=1e-6, atol=1e-6)
    cache = {i: ([seeded_randn((1, 8, 4, 4), 600 + 10 * i + k) for k in range(3)], seeded_randn((1, 8, 2, 2), 700 + i)) for i in range(6)}
    down, mid = pipe.select_controlnet_res_samples(cache, [[0, 1], [4, 5]], True, 4, 2)
    assert all(torch.equal(d, g[f"select/down{k}"]) for k, d in enumerate(down)) and torch.equal(mid, g["select/mid"])


def test_nearest_index_helper_is_torchs_nearest_resize():
    """tests/test_gpu_conv_loader.py builds the reference of the explicit-size upsampling (emo_gemm_params.up_h / up_w) with
    `nearest_index`: it must be F.interpolate(size=..., mode="nearest") itself - on an index ramp, so that the output IS the source
    index - for every in < 130 and in <= out <= 4 in.  The integer dst * in / out, which the conv loader used to compute, is not: it
    agrees for out = 2 in and 2 in - 1 (the sizes the UNet asks for) and differs at hundreds of other pairs, e.g. 14 -> 46 at dst 23."""
    import torch.nn.functional as F
    from tests.test_gpu_conv_loader import nearest_index
    differs = 0
    for n_in in range(1, 130):
        ramp = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, n_in, 1)
        for n_out in range(n_in, 4 * n_in + 1):
            want = F.interpolate(ramp, size=(n_out, 1), mode="nearest").reshape(-1).to(torch.int64)
            got = nearest_index(n_in, n_out)
            assert torch.equal(got, want), (n_in, n_out)
            integer = torch.arange(n_out) * n_in // n_out
            if n_out in (2 * n_in, 2 * n_in - 1):
                assert torch.equal(integer, want), (n_in, n_out)
            differs += int(not torch.equal(integer, want))
    assert differs == 625
    assert nearest_index(14, 46)[23] == 6 and nearest_index(26, 44)[22] == 12 and nearest_index(21, 69)[[23, 46]].tolist() == [6, 13]


def test_attention_sweeps_reach_every_instantiation():
    """emo_attention_plan (csrc/attention.hip: the launch chain run without a launch) against the shapes that
    tests/test_gpu_attention_sweeps.py launches: the sweep must reach every (head-dim class, loader rounds, ring depth) the library
    can pick for an admissible head dim - taken from the library, so a later change to the classes cannot silently shrink the
    coverage -, its "resident" shapes must take the resident walk (q tiles per block > 1) and its "streaming" shapes must not."""
    from tests import attention_sweep_cases as S
    counts = {}
    for dtype in S.DTYPES:
        dims = S.head_dims(dtype)
        # every instantiation an admissible head dim can reach (class, rounds and ring depth follow from d and the dtype alone:
        # asked on a one-tile and on a many-tile shape, with and without a second segment, causal or not)
        reachable = set()
        for d in dims:
            for kw in (dict(B=1, Lq=1, Lk0=1, heads=1), dict(B=3, Lq=1000, Lk0=1000, heads=5, Lk1=300),
                       dict(B=2, Lq=64, Lk0=64, heads=2, causal=True)):
                reachable.add(S.plan(dtype, d, **kw)[:3])
        swept = set()
        for d in dims:
            per_d = set()
            for kw in S.streaming_shapes(d):
                pl = S.plan(dtype, d, **kw)
                assert pl[3] == 1, (dtype, d, kw, pl)
                assert pl[4] == int(bool(kw.get("causal"))), (dtype, d, kw, pl)
                per_d.add(pl[:3])
            for kw in S.resident_shapes(d):
                pl = S.plan(dtype, d, **kw)
                assert pl[3] == S.RESIDENT_LQ[kw["Lq"]] > 1, (dtype, d, kw, pl)
                per_d.add(pl[:3])
            assert len(per_d) == 1, (dtype, d, per_d)      # one head dim = one instantiation, whatever the shape
            swept |= per_d
        assert swept == reachable, (dtype, swept ^ reachable)
        counts[dtype] = len(swept)
        # the ring-schedule matrix runs two ring depths per dtype, the shallowest one the dtype has among them
        ring = {S.plan(dt_, d, B=4, Lq=130, Lk0=64, heads=2)[2] for dt_, d in S.RING if dt_ == dtype}
        assert len(ring) == 2 and min(ring) == min(pl[2] for pl in reachable), (dtype, ring)
        # the causal resident walk exists for some head dim (the sweep launches it wherever the plan reports it)
        c = S.CAUSAL_RESIDENT
        assert any(S.plan(dtype, d, B=c["B"], Lq=c["L"], Lk0=c["L"], heads=c["heads"], causal=True)[3] > 1 for d in dims)
    # more than a handful each (2-byte: 12, f32: 18 when this test was written - not pinned: the library is the authority)
    assert all(n >= 6 for n in counts.values()), counts
    ring_all = {S.plan(dt_, d, B=4, Lq=130, Lk0=64, heads=2)[2] for dt_, d in S.RING}
    assert ring_all == {1, 2, 3}


def test_attention_plan_runs_the_argument_checks():
    """emo_attention_plan returns what emo_attention's argument checks return, and writes nothing on a refusal."""
    import ctypes as C
    from emote_hack_amd import ops
    from emote_hack_amd._lib import AttentionParams, EmoHipError
    with pytest.raises(EmoHipError):
        ops.attention_plan(dtype=torch.bfloat16, B=2, Lq=64, Lk0=64, heads=2, d=44)        # d % 8
    with pytest.raises(EmoHipError):
        ops.attention_plan(dtype=torch.float32, B=2, Lq=64, Lk0=64, heads=2, d=164)         # above 160
    with pytest.raises(EmoHipError):
        ops.attention_plan(dtype=torch.float16, B=2, Lq=64, Lk0=65, heads=2, d=64, causal=True)   # causal needs Lq == Lk0
    with pytest.raises(EmoHipError):
        ops.attention_plan(dtype=torch.float16, B=2, Lq=64, Lk0=64, heads=2, d=64, Lk1=8, causal=True)
    lib = _lib.load()
    plan = (C.c_int * 5)(-7, -7, -7, -7, -7)
    assert lib.emo_attention_plan(C.byref(AttentionParams()), plan) != 0      # null pointers
    assert lib.emo_attention_plan(None, plan) != 0
    assert list(plan) == [-7] * 5
    assert ops.attention_plan(dtype=torch.bfloat16, B=24, Lq=4096, Lk0=77, heads=8, d=40)[3] == 4   # the text cross-attention of the 64x64 level
    assert ops.attention_plan(dtype=torch.bfloat16, B=24, Lq=4096, Lk0=4096, heads=8, d=40, Lk1=4096) == (6, 3, 3, 1, 0)


def test_gemm_sweeps_reach_every_instantiation():
    """emo_gemm_plan (csrc/gemm.hip: emo_gemm's checks, planner and launch chain run without a launch) against the case tables that
    tests/test_gpu_gemm_sweeps.py launches: they must reach every dense instantiation dispatch_gemm / dispatch_tile can produce -
    tile x {plain, V^T, LayerNorm fold, fold + V^T} x dtype minus what the `if constexpr` guards of dispatch_tile exclude -, both main
    loops, every store path on every tile that can take it, and the bias / row bias both in and out of the accumulators.  The path
    reported comes from the predicates the kernels themselves evaluate (csrc/gemm_api.h), so a table that shrinks fails here."""
    from emote_hack_amd import ops
    from tests import gemm_sweep_cases as S
    paths = {n: i for i, n in enumerate(ops.GEMM_STORE_PATHS)}
    seen, stores, loops, in_acc, vt_split = set(), set(), set(), set(), set()
    n_cases = 0
    for _name, cases in S.all_tables():
        for c in cases:
            fam, tile, phase, flags, split, store, b_acc, rb_acc = S.plan(c)
            n_cases += 1
            assert fam == 0 and not flags & 1, c                  # dense, the tile kernel
            assert phase == int(tile == 7), (c, tile, phase)
            assert split == (c.get("split_k", 1) or split), c
            two = c["dtype"] != torch.float32
            seen.add((c["dtype"], tile, flags & 6))
            stores.add((two, tile, flags & 2, store))
            loops.add(phase)
            in_acc.add((b_acc, rb_acc))
            if flags & 8:
                vt_split.add((c["dtype"], tile))
    # every instantiation: the guards of dispatch_tile leave 256x160 to the row-major kernels, 256x320 and the phase loop to the
    # row-major 2-byte ones (plan_gemm and dispatch_tile send the other hints to 128x160 / 128x128 / 256x256)
    excluded = {(dt_, t, f) for dt_ in S.DTYPES for t in (5, 6, 7) for f in (2, 6)} | {(torch.float32, t, f) for t in (6, 7) for f in (0, 4)}
    want = {(dt_, t, f) for dt_ in S.DTYPES for t in range(1, 8) for f in (0, 2, 4, 6)} - excluded
    assert len(excluded) == 22 and seen == want, (want - seen, seen - want)
    assert loops == {0, 1}
    want_stores = set()
    for two in (False, True):
        row_tiles = range(1, 8) if two else range(1, 6)
        for t in row_tiles:
            want_stores |= {(two, t, 0, paths[s]) for s in (("lds",) if two else ()) + ("vec_row", "scalar_row")}
            if t != 7:      # (split-K takes the lockstep loop)
                want_stores.add((two, t, 0, paths["splitk_ws"]))
        want_stores |= {(two, t, 2, paths[s]) for t in (1, 2, 3, 4) for s in ("vt_quad", "vt_scalar", "splitk_ws")}
    assert stores == want_stores, (want_stores - stores, stores - want_stores)
    assert in_acc == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {t for _, t in vt_split} >= {1, 2} and {d for d, _ in vt_split} == set(S.DTYPES)
    assert n_cases >= 14000       # (14472 when this test was written: the tables are the sweep)
    # the fallbacks of a pinned tile
    pl = lambda **kw: ops.gemm_plan(M=512, N=320, **kw)
    for dt_ in (torch.bfloat16, torch.float16):
        assert pl(dtype=dt_, K=128, tile=7)[1:3] == (7, 1)
        assert pl(dtype=dt_, K=128 + 8, tile=7)[1:3] == (4, 0)          # ragged K
        assert pl(dtype=dt_, K=64, tile=7)[1:3] == (4, 0)               # one stage: the phase loop needs two
        assert pl(dtype=dt_, K=640, tile=7, split_k=2)[1:3] == (4, 0)
        assert pl(dtype=dt_, K=128, tile=6)[1] == 6 and pl(dtype=dt_, K=128, tile=5)[1] == 5
        assert pl(dtype=dt_, K=128, tile=5, transpose_rows=64, transpose_ld=64)[1] == 3
    assert pl(dtype=torch.float32, K=128, tile=7)[1:3] == (4, 0)
    assert pl(dtype=torch.float32, K=128, tile=6)[1] == 3                # 256x320 is 2-byte only: 128x160
    for hint in (8, 9, 15):
        assert pl(dtype=torch.bfloat16, K=128, tile=hint)[1] == 2        # above the table: 128x128
    # GEGLU pairs value and gate tiles inside a wave: even wave widths only
    assert {ops.gemm_plan(dtype=torch.bfloat16, M=512, N=320 * 2, K=128, geglu=True, tile=t)[1] for t in (1, 3, 5, 6)} == {2}
    # the conv loader: the halo family where it serves, else the tile kernel with the conv flag (hints 5 / 6 fall back to 128x128)
    conv = dict(H=16, W=16, Cin=64, stride=1, Ho=16, Wo=16)
    assert ops.gemm_plan(dtype=torch.bfloat16, M=512, N=128, K=576, conv=conv, split_k=1) == (1, 0, 0, 0, 0, 0, 0, 0)
    conv2 = dict(H=16, W=16, Cin=64, stride=2, Ho=8, Wo=8)
    assert ops.gemm_plan(dtype=torch.bfloat16, M=128, N=128, K=576, conv=conv2, tile=5, split_k=1)[:4] == (0, 2, 0, 1)


def test_planner_can_pick_a_split_with_an_empty_slice():
    """plan_gemm caps the split at nk / 4 slices but cuts K into slices of ceil(nk / s) stages: (s - 1) * ceil(nk / s) >= nk leaves the
    last slice without a stage (nk = 25 split 6 ways: 5 slices of 5).  The kernel must then write zeros to that slab
    (tests/test_gpu_gemm_sweeps.py runs what this search finds).  The search covers the planner's splitting domain - few-tile dense
    shapes, nk = 8 .. 400 stages, every dtype - and must keep finding the short-K hit and report the long-K ones."""
    from tests import gemm_sweep_cases as S
    hits = S.planned_empty_slices()
    assert any(h["_nk"] == 25 and h["_S"] == 6 for h in hits)
    assert all(S.split_empty(h["_nk"], h["_S"]) and h["_S"] <= h["_nk"] // 4 for h in hits)
    for h in hits[:50]:
        assert S.plan({k: v for k, v in h.items() if not k.startswith("_")})[4] == h["_S"]
    long_k = sorted({(h["_nk"], h["_S"]) for h in hits if h["_nk"] >= 41})
    print(f"planned splits with an empty slice: {len(hits)} of the searched shapes; nk >= 41: {long_k[:12]}")


def test_window_gemm_sweeps_reach_every_tile_with_lda_below_k():
    """emo_gemm_plan over the window-GEMM tables of tests/frontend_sweep_cases.py (tests/test_gpu_frontend_gemm_sweeps.py launches
    them): with lda < K they must reach every tile instantiation 1 .. 7, both main loops and the split-K workspace store; and the
    GEMMs wav2vec2-base runs at 1 s and 10 s of audio - feature-encoder layers of M = 3199 / 31999 rows and below, N = 512,
    K = 16 / 1536 / 1024, the positional conv at T = 49 / 499 - must each map to a (tile, main loop, split or not) of their dtype
    that the tables contain."""
    from emote_hack_amd import ops
    from tests import frontend_sweep_cases as S
    ws = ops.GEMM_STORE_PATHS.index("splitk_ws")
    below, combos, n_cases = set(), set(), 0
    for _name, cases, plan in S.win_tables():
        assert cases
        for c in cases:
            fam, tile, phase, flags, split, store, _b_acc, _rb_acc = plan(c)
            n_cases += 1
            assert fam == 0 and flags == 0, c                                    # dense, the row-major tile kernel
            assert phase == int(tile == 7) and (split > 1) == (store == ws), (c, tile, phase, split, store)
            if c["split_k"] is not None:
                assert split == c["split_k"], c
            combos.add((c["dtype"], tile, phase, split > 1))
            if c["lda"] < c["K"]:
                below.add((tile, phase, split > 1))
    assert n_cases == 3 * (4 * 3 * 2 * 8 * 3 * 2 + 3 * 2 * 3 * 2)
    assert {t for t, _, _ in below} == set(range(1, 8)) and {p for _, p, _ in below} == {0, 1}
    assert any(s for _, _, s in below)                                           # plan[4] > 1 on store path 5
    assert any(c["split_k"] is None and plan(c)[4] > 1 for _n, cases, plan in S.win_tables() for c in cases if c["lda"] < c["K"])
    for n_samples, rows, frames in ((16000, 3199, 49), (160000, 31999, 499)):
        gemms = S.base_model_gemms(n_samples)
        assert gemms[0] == (rows, 512, 16, 16) and gemms[1][1:] == (512, 1536, 1024) and gemms[6] == (frames, 512, 1024, 1024)
        assert gemms[7] == (frames, 48, 6144, 48) and {g[2] for g in gemms[:7]} == {16, 1536, 1024}
        for dtype in S.DTYPES:
            for i, (M, N, K, lda) in enumerate(gemms):
                p = ops.gemm_plan(dtype=dtype, M=M, N=N, K=K, lda=lda, bias=i == 7, split_k=None)      # what Wav2Vec2Model.forward asks
                assert (dtype, p[1], p[2], p[4] > 1) in combos, (n_samples, dtype, (M, N, K, lda), p)


def test_window_gemm_probes_are_exact():
    """The exact probes of the window GEMMs (tests/frontend_sweep_cases.py win_operands / pos_operands assert it while they build):
    every expected sum is a multiple of 1/16 below 16, representable in f32, f16 and bf16 - so is every partial sum, in any order."""
    from tests import frontend_sweep_cases as S
    for dtype in S.DTYPES:
        for key in S.win_keys(dtype):
            op = S.win_operands(dtype, *key, "probe")
            k, s, C, M = key
            # the closed form against the convolution it restates
            ref = torch.nn.functional.conv1d(op["x"].double().t()[None], op["w"].double().view(-1, k, C).permute(0, 2, 1), stride=s)[0].t()
            assert torch.equal(ref, op["y0"]), key
            assert op["x"].shape == ((M - 1) * s + k, C) and bool((op["x"].sum(1) == 1).all())
        for key in S.pos_keys(dtype):
            S.pos_operands(dtype, *key, "probe")
    assert [S.cn_chunks(x) for x in (1, 256, 257, 514, 16384, 16385, 33000)] == [(1, 1, 1), (1, 256, 16), (2, 129, 17), (3, 172, 33),
                                                                                 (64, 256, 512), (64, 257, 512), (64, 516, 512)]


def test_halo_sweeps_reach_every_instantiation():
    """emo_conv3x3_halo_plan (csrc/gemm.hip plan_halo: the function the launch path decides by, asked without a launch) against the
    case tables that tests/test_gpu_conv_halo_sweeps.py launches.  Every case must be served by the halo-reuse kernel with the patch
    height and the block widths it names; every "many tiles" launch must give every block two tiles and some three
    (tiles >= 2 * grid + 1); together the cases must reach all 27 instantiations of gemm_run_halo and, in the many-tile launches,
    both branches of the kernel's tile_of (tiles % 8 zero and not) and both halo-buffer parities from tile to tile (odd and even
    chunk counts).  A table that shrinks, or a planner change that moves a case to another kernel, fails here."""
    from emote_hack_amd import ops
    from tests import halo_sweep_cases as H
    seen, many_mod8, many_chunks = set(), set(), set()
    for name, cases in H.all_tables():
        assert cases, name
        for case in cases:
            c = H.full(case)
            for dtype in H.DTYPES:
                served, ph, bn_a, tiles_a, grid_a, bn_b, tiles_b, grid_b = H.plan(case, dtype)
                assert served == 1, (name, case, dtype)                                                     # (a)
                assert (ph, bn_a, bn_b) == (c["ph"], c["main"], c["tail"]), (name, case, dtype, ph, bn_a, bn_b)   # (b)
                for which, bn, tiles, grid in (("main", bn_a, tiles_a, grid_a), ("tail", bn_b, tiles_b, grid_b)):
                    if not bn:
                        assert (tiles, grid) == (0, 0) and which not in c["many"], (name, case)
                        continue
                    assert grid == min(tiles, H.GRID[ph]), (name, case, tiles, grid)
                    seen.add((dtype, ph, bn, c["gn"]))
                    if which in c["many"]:
                        assert tiles >= 2 * grid + 1, (name, case, dtype, which, tiles, grid)              # (c)
                        many_mod8.add(tiles % 8 == 0)
                        many_chunks.add(c["chunks"] % 2)
                        # the walk of the table's tile_of covers every tile once, and the first block walks three
                        walk = sorted(H.tile_of(i, tiles) for i in range(tiles))
                        assert walk == list(range(tiles)) and len(range(0, tiles, grid)) >= 3
            if name in ("many", "gn_many"):
                assert c["many"], (name, case)
    want = {(dtype, ph, bn, gn) for dtype in H.DTYPES for ph in (8, 16) for bn in (128, 64) for gn in (False, True)}
    want |= {(dtype, 16, 192, False) for dtype in H.DTYPES}
    assert len(want) == 27 and seen == want, (want - seen, seen - want)                                     # (d)
    assert many_mod8 == {True, False} and many_chunks == {0, 1}                                             # (e)
    # the in-place residual on a ragged frame is NOT the halo kernel's (two blocks store the overlapped pixels): the conv loader's
    for case in H.INPLACE_RAGGED:
        for dtype in H.DTYPES:
            assert H.plan(case, dtype) == (0,) * 8, (case, dtype)
            assert H.plan(dict(case, residual=1), dtype)[0] == 1         # ... the alias is the only reason
            g = H.geometry(case, dtype)
            conv = dict(H=case["H"], W=case["W"], Cin=g["Cin"], stride=1, Ho=case["H"], Wo=case["W"])
            fam, _tile, _phase, flags = ops.gemm_plan(dtype=dtype, M=case["n"] * case["H"] * case["W"], N=case["N"], K=9 * g["Cin"], conv=conv,
                                                      bias=True, residual=True, split_k=1)[:4]       # (gemm_plan's residual aliases C)
            assert fam == 0 and flags & 1, (case, dtype)
    # emo_gemm_plan keeps its answer for the family, and the new entry runs emo_gemm's checks
    assert ops.gemm_plan(dtype=torch.bfloat16, M=512, N=128, K=576, conv=dict(H=16, W=16, Cin=64, stride=1, Ho=16, Wo=16), split_k=1) == (1, 0, 0, 0, 0, 0, 0, 0)
    assert ops.conv_halo_plan(dtype=torch.bfloat16, n_img=2, H=16, W=16, Cin=64, N=128) == (1, 8, 128, 4, 4, 0, 0, 0)
    assert ops.conv_halo_plan(dtype=torch.bfloat16, n_img=2, H=16, W=16, Cin=64, N=320, tile=2) == (1, 16, 128, 2, 2, 192, 2, 2)
    assert ops.conv_halo_plan(dtype=torch.bfloat16, n_img=2, H=16, W=8, Cin=64, N=128) == (0,) * 8          # 8-pixel rows: the im2col loader
    assert ops.conv_halo_plan(dtype=torch.bfloat16, n_img=200, H=16, W=16, Cin=64, N=128)[1] == 16          # 200 tiles of 16 rows: planned
    with pytest.raises(_lib.EmoHipError):
        ops.conv_halo_plan(dtype=torch.bfloat16, n_img=2, H=16, W=16, Cin=60, N=128)                        # Cin % 8
    with pytest.raises(_lib.EmoHipError):
        ops.conv_halo_plan(dtype=torch.bfloat16, n_img=2, H=16, W=8, Cin=64, N=128, gn=True)                # the fold needs the halo kernel
    import ctypes as C
    plan = (C.c_int * 8)(*([-7] * 8))
    assert _lib.load().emo_conv3x3_halo_plan(C.byref(_lib.GemmParams()), plan) != 0 and list(plan) == [-7] * 8
    assert _lib.load().emo_conv3x3_halo_plan(None, plan) != 0


def _gn_plan(N, S, Cc, G, dt):
    import ctypes as C
    plan = (C.c_int * 12)(*([-7] * 12))
    return _lib.load().emo_groupnorm_plan(N, S, Cc, G, dt, plan), tuple(plan)


def _ln_plan(M, Cc, dt):
    import ctypes as C
    plan = (C.c_int * 4)(*([-7] * 4))
    return _lib.load().emo_layernorm_plan(M, Cc, dt, plan), tuple(plan)


def test_norm_sweeps_reach_every_arm():
    """emo_groupnorm_plan / emo_layernorm_plan (csrc/norm.hip: the gn_geom / gn1_geom / ln_geom the launches call, asked without a
    launch) against the case tables tests/test_gpu_norm_sweeps.py launches: every case plans what it was written for in every dtype of
    its class, the one-launch query and the workspace size agree with the plan, and between them the tables reach the wide arm, every
    column split, both chunk-count mismatches, the empty chunks, the group extremes, every (threads, rows per thread, groups per slab)
    of the one-launch kernel and every lanes-per-row choice of the LayerNorm at a partly filled wavefront and past the grid.  A table
    that shrinks, or a retuning that moves a case to another arm, fails here."""
    from tests import norm_sweep_cases as S
    lib = _lib.load()
    arms, one_shapes = set(), {"h": set(), "f": set()}
    for c in S.GN:
        N, Sr, Cc, G = c["N"], c["S"], c["C"], c["G"]
        for dtype in S.CLASS_DTYPES[c["cls"]]:
            rc, plan = _gn_plan(N, Sr, Cc, G, _dt(dtype))
            assert rc == 0 and plan == c["two"] + c["one"], (S.gn_id(c), dtype, plan)
            assert lib.emo_groupnorm_one_launch_ok(N, Sr, Cc, G, _dt(dtype)) == plan[6]
        # sized for the larger chunk count of the two vector widths - of those that divide C (C = 4, an f32-only row, used to divide by zero)
        ns = max(_gn_plan(N, Sr, Cc, G, _dt(dtype))[1][3] for dtype in (torch.bfloat16, torch.float32) if Cc % S.vec(S.cls_of(dtype)) == 0)
        assert lib.emo_groupnorm_workspace_bytes(N, Sr, Cc, G) == N * ns * G * 8
        NC, Cp, RP, n_s, n_a, wide = c["two"]
        assert NC * Cp == Cc and wide == (Cp // S.vec(c["cls"]) > S.GN_THREADS) and n_s <= 256 and n_s <= n_a
        assert S.gn_max_chunk_elems(c) * 16 < 2 ** 24       # the grid probe's integer sums (|x| <= 4) stay exact in an f32 partial
        assert N * Sr * Cc * (2 if c["cls"] == "h" else 4) <= 50e6
        arms |= S.gn_arms(c)
        if c["one"][0]:
            ok, gpb, Wc, NT, R, slots = c["one"]
            assert Wc == gpb * (Cc // G) and slots == NT // (Wc // S.vec(c["cls"])) and -(-Sr // slots) <= R
            one_shapes[c["cls"]].add((NT, R, gpb))
    assert arms == S.GN_TWO_ARMS, (arms ^ S.GN_TWO_ARMS)
    assert one_shapes == S.GN_ONE_SHAPES, {k: one_shapes[k] ^ S.GN_ONE_SHAPES[k] for k in one_shapes}
    # the two instantiations the workload never launches: 16 rows per thread (f32) and 8 rows per thread in a 2-byte type
    assert any(c["cls"] == "f" and c["one"][4] == 16 for c in S.GN) and any(c["cls"] == "h" and c["one"][4] == 8 for c in S.GN)
    assert S.gn_rerun_as_views(next(c for c in S.GN if c["name"] == "split")) and not S.gn_rerun_as_views(next(c for c in S.GN if c["name"] == "idle"))

    seen = set()
    for c in S.LN:
        M, Cc = c["M"], c["C"]
        for dtype in S.CLASS_DTYPES[c["cls"]]:
            rc, plan = _ln_plan(M, Cc, _dt(dtype))
            assert rc == 0 and plan == c["plan"], (S.ln_id(c), dtype, plan)
        lpr, rpw, grid, second = c["plan"]
        assert lpr * rpw == 64 and grid == min(-(-M // (4 * rpw)), S.LN_MAXGRID) and second == (M > S.LN_MAXGRID * 4 * rpw)
        assert M * Cc * (2 if c["cls"] == "h" else 4) <= 51e6
        kinds = {"one_row"} if M == 1 else set()
        if M % rpw:
            kinds.add("ragged_wave")
        if M % (4 * rpw):
            kinds.add("ragged_block")
        if second:
            kinds.add("second_trip")
        if Cc // S.vec(c["cls"]) == S.LN_MAXV * lpr:
            kinds.add("full_lanes")
        seen |= {(c["cls"], lpr, k) for k in kinds}
    # (64 lanes per row: a wavefront holds one row and is never partly filled - its last BLOCK is, at M = 2)
    assert seen == {(cls, lpr, k) for cls in "hf" for lpr in S.LN_LPRS for k in ("one_row", "ragged_wave", "ragged_block", "second_trip", "full_lanes")
                    if not (lpr == 64 and k == "ragged_wave")}


def test_norm_plans_run_the_argument_checks():
    """emo_groupnorm_plan returns what the GroupNorm entries' shape check returns and emo_layernorm_plan what the LayerNorm's returns,
    and neither writes anything on a refusal; the fold keeps its own width limit."""
    import ctypes as C
    from tests import norm_sweep_cases as S
    lib = _lib.load()
    for N, Sr, Cc, G, cls in S.GN_REFUSED:
        for dtype in S.CLASS_DTYPES[cls]:
            rc, plan = _gn_plan(N, Sr, Cc, G, _dt(dtype))
            assert rc != 0 and plan == (-7,) * 12, (N, Sr, Cc, G, dtype)
            assert lib.emo_groupnorm_one_launch_ok(N, Sr, Cc, G, _dt(dtype)) == 0
            # the launching entries refuse the same shapes in their checks, before they touch a pointer (these are not dereferenced)
            buf = (C.c_float * 16)()
            p = C.addressof(buf)
            assert lib.emo_groupnorm_stats(p, Cc, p, N, Sr, Cc, G, _dt(dtype), None) == rc
            assert lib.emo_groupnorm_apply(p, Cc, p, p, p, p, Cc, N, Sr, Cc, G, 1e-5, 0, _dt(dtype), None) == rc
            assert lib.emo_groupnorm(p, Cc, p, p, p, Cc, N, Sr, Cc, G, 1e-5, 0, _dt(dtype), None) == rc
            assert lib.emo_groupnorm_coeffs(p, p, p, p, N, Sr, Cc, G, 1e-5, _dt(dtype), None) == rc
    assert _gn_plan(2, 37, 320, 32, 7)[0] != 0 and _gn_plan(0, 37, 320, 32, BF16)[0] != 0 and _gn_plan(2, 0, 320, 32, BF16)[0] != 0
    assert lib.emo_groupnorm_plan(2, 37, 320, 32, BF16, None) != 0
    assert lib.emo_groupnorm_workspace_bytes(32, 1, 4, 4) == 32 * 4 * 8 and lib.emo_groupnorm_workspace_bytes(2, 37, 0, 4) == 0
    # 768 column vectors, 128 groups: the last shapes served
    assert _gn_plan(2, 37, 768 * 8, 128, BF16)[0] == 0 and _gn_plan(2, 37, 768 * 4, 128, F32)[0] == 0
    # the fold: C <= 2560 (its LDS tables), whatever the plan says of the norm itself
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    for dt, V in ((BF16, 8), (F32, 4)):
        assert _gn_plan(2, 50, S.GNF_MAXC + 32, 32, dt)[0] == 0
        assert lib.emo_groupnorm_fold_linear(p, p, p, p, None, p, p, 2, 50, S.GNF_MAXC + 32, 32, 13, 1e-6, dt, None) != 0
    for dt, V in ((BF16, 8), (_dt(torch.float16), 8), (F32, 4)):
        assert _ln_plan(0, 64, dt) == (_ln_plan(0, 64, dt)[0], (-7,) * 4) and _ln_plan(0, 64, dt)[0] != 0
        assert _ln_plan(5, 64 + V // 2, dt)[0] != 0 and _ln_plan(5, (64 * S.LN_MAXV + 1) * V, dt)[0] != 0
        assert _ln_plan(5, 64 * S.LN_MAXV * V, dt) == (0, (64, 1, 2, 0))
        assert lib.emo_layernorm(p, 64, p, p, p, 64, 0, 64, 1e-5, None, 0, 0, dt, None) == _ln_plan(0, 64, dt)[0]
        assert lib.emo_layernorm_stats(p, (64 * S.LN_MAXV + 1) * V, p, 5, (64 * S.LN_MAXV + 1) * V, 1e-5, dt, None) == _ln_plan(5, (64 * S.LN_MAXV + 1) * V, dt)[0]
    assert _ln_plan(5, 64, 7)[0] != 0 and lib.emo_layernorm_plan(5, 64, BF16, None) != 0


def test_elementwise_sweep_cases_are_what_they_are_named_for():
    """tests/elementwise_sweep_cases.py against the launch geometry of csrc/elementwise.hip, redone here: which layout cases have a ragged
    pixel tile, a channel tile of padding only, and more tiles than the transposes launch blocks; which cases of the grid-stride
    entries take a second (or third) trip; which sampler-step cases take the float4 path.  And the refusals of the layout pair: they
    return before anything is launched, so they run here with pointers that are never dereferenced."""
    import ctypes as C
    from tests import elementwise_sweep_cases as E
    by = {E.layout_id(c): c for c in E.LAYOUT}
    assert len(by) == len(E.LAYOUT) == 7
    tiles = {k: E.layout_tiles(c) for k, c in by.items()}
    assert tiles["C5-Cpad8-B2-F3-H6-W10"] == (1, 1, 6)
    assert tiles["C32-Cpad40-B1-F2-H7-W9"][1] == 2 and E.layout_tiles(by["C32-Cpad40-B1-F2-H7-W9"], to_rows=False)[1] == 1
    assert tiles["C33-Cpad40-B2-F1-H5-W13"][:2] == (2, 2) and 5 * 13 == E.LAYOUT_TILE_P + 1
    assert tiles["C31-Cpad32-B1-F2-H9-W7"][:2] == (1, 1) and 9 * 7 == E.LAYOUT_TILE_P - 1
    assert tiles["C64-Cpad64-B1-F1-H8-W8"] == (1, 2, 2)
    assert tiles["C4-Cpad8-B1-F1-H1-W1"] == (1, 1, 1)
    for to_rows in (True, False):
        pt, ct, n = E.layout_tiles(E.LAYOUT_WALK, to_rows)
        assert (pt, ct, n) == (2049, 2, 4098) and n > E.LAYOUT_MAX_BLOCKS
    assert sum(E.layout_tiles(c)[2] > E.LAYOUT_MAX_BLOCKS for c in E.LAYOUT) == 1
    # grid-stride entries: work items of each named case against one trip of the capped grid
    assert E.trips(E.ONE_TRIP) == 1 and E.trips(E.ONE_TRIP + 1) == 2
    assert E.TS_WALK["B"] * E.TS_WALK["dim"] == 526119 and E.trips(526119) == 2
    assert [E.trips(n) for n in E.SILU_SIZES] == [1, 1, 1, 3] and E.SILU_SIZES[-1] % E.BLOCK != 0
    w = E.COPY_ADD_WALK
    assert w["M"] * (w["C"] // E.vec(torch.float32)) == 524672 and E.trips(524672) == 2 and w["ld"] % 4 == 0 and w["ld"] > w["C"]
    w = E.ADD_PERIODIC_WALK
    assert w["P"] * w["periods"] == 65541 and E.trips(65541 * (w["C"] // E.vec(torch.bfloat16))) == 2
    assert E.trips(E.CONVERT_WALK) == 3
    w = E.ACCUMULATE_WALK
    assert w["nf"] * w["C"] * w["HW"] == 524400 and E.trips(524400) == 2 and len(w["frames"]) == w["nf"] and max(w["frames"]) < w["F"]
    for C_, F, HW in E.SCHED_SMALL:
        assert (C_ * F * HW) % 4 == 0 and (HW < 4 or F == 1)
    (C_, F, HW), (C2, F2, HW2) = E.SCHED_LARGE
    assert C_ * F * HW == 2097252 and (C_ * F * HW) % 4 == 0 and E.trips(C_ * F * HW // 4) == 2 and HW % 4 == 3
    assert C2 * F2 * HW2 == 524289 and (C2 * F2 * HW2) % 4 != 0 and E.trips(524289) == 2
    # refusals of the layout pair
    lib = _lib.load()
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    for c in E.LAYOUT:
        B, F, H, W = c["shape"]
        for entry, over in E.layout_refusals(c):
            a = dict(B=B, C=c["C"], F=F, H=H, W=W, Cpad=c["Cpad"], ldo=c["Cpad"], ldi=c["C"])
            a.update(over)
            if entry == "to_rows":
                rc = lib.emo_ncfhw_to_rows(p, p, a["B"], a["C"], a["F"], a["H"], a["W"], a["Cpad"], a["ldo"], BF16, None)
            else:
                rc = lib.emo_rows_to_ncfhw(p, p, a["B"], a["C"], a["F"], a["H"], a["W"], a["ldi"], BF16, None)
            assert rc != 0, (entry, over)
