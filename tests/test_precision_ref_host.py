"""CPU side of the precision gate (tests/test_gpu_precision.py): the measures of tests/precision_ref.py are right, the CPU f32 MODEL of
every contract meets the GPU file's own condition on the GPU file's own inputs with room (a quarter of each share cap, inside every
budget), and the MUTANTS - one added intermediate rounding, a lowered accumulator, a truncation - each FAIL the condition of their
family while they PASS the blanket TOL of tests/test_gpu_kernels.py.  That is the argument for the gate, kept executable."""
import pytest
import torch

from tests import precision_ref as P
from tests import test_gpu_precision as G
from tests.test_gpu_kernels import TOL          # the blanket tolerances the mutants must PASS: the kernel suite's own

ROOM = 0.25                                     # the models keep a quarter of each cap


def passes_old_tol(got, r, dtype):
    try:
        torch.testing.assert_close(got.float(), r.float(), **TOL[dtype])
        return True
    except AssertionError:
        return False


# ---- the measures -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", G.DTYPES, ids=G.IDS)
def test_ulp_and_one_step_rounding(dtype):
    fi = torch.finfo(dtype)
    mant = P.MANT[dtype]
    one = torch.tensor([1.0, 1.5, 2.0, 0.75, -3.0, 0.0, fi.smallest_normal, fi.smallest_normal / 4, fi.max, float("inf")], dtype=torch.float64)
    want = [2.0 ** -mant, 2.0 ** -mant, 2.0 ** (1 - mant), 2.0 ** (-1 - mant), 2.0 ** (1 - mant)] + [fi.smallest_normal * 2.0 ** -mant] * 3 + \
           [2.0 ** (P.EMAX[dtype] - mant)] * 2
    assert P.ulp(one, dtype).tolist() == want
    # every f32 value rounds as torch's own one-step cast from f32 does
    x = torch.cat([torch.randn(20000, generator=G.gen(1)) * 3, torch.randn(5000, generator=G.gen(2)) * 1e-6 * fi.smallest_normal / 6e-5,
                   torch.tensor([fi.max, -fi.max, 0.0, -0.0, float("inf"), -float("inf")]), torch.randn(2000, generator=G.gen(3)) * fi.max / 3])
    got, ref = P.correctly_rounded(x.double(), dtype), x.to(dtype)
    assert got.dtype == dtype and torch.equal(got.float().view(torch.int32), ref.float().view(torch.int32))
    assert bool(torch.isnan(P.correctly_rounded(torch.tensor([float("nan")]), dtype)).all())
    if dtype != torch.float32:
        # ties go to even, and a value just above a tie goes up although its f32 image IS the tie (torch's f64 cast double-rounds)
        u = 2.0 ** -mant
        t = torch.tensor([1 + u / 2, 1 + 3 * u / 2, 1 + u / 2 + 2.0 ** -40, fi.max + 2.0 ** (P.EMAX[dtype] - mant - 1)], dtype=torch.float64)
        assert P.correctly_rounded(t, dtype).double().tolist() == [1.0, 1 + 2 * u, 1 + u, float("inf")]
        assert float(t[2].to(dtype)) == 1.0                   # why correctly_rounded exists


def test_misrounded_share_and_ratios():
    r = torch.tensor([1.0, 1.00390625, 0.0, 70000.0, 0.3], dtype=torch.float64)
    good = P.correctly_rounded(r, torch.float16)
    assert good.tolist() == [1.0, 1.00390625, 0.0, float("inf"), 0.300048828125]
    assert P.misrounded_share(good, r) == 0.0
    assert P.misrounded_share(torch.tensor([1.0, 1.00390625, -0.0, float("inf"), 0.300048828125], dtype=torch.float16), r) == 0.0     # +-0
    assert P.misrounded_share(torch.tensor([1.0, 1.0048828125, 0.0, float("inf"), 0.2998046875], dtype=torch.float16), r) == 0.5      # 2 of 4
    with pytest.raises(AssertionError):
        P.misrounded_share(torch.tensor([1.0, 1.00390625, 0.0, 65504.0, 0.3], dtype=torch.float16), r)                               # inf is exact
    model, got = r + 1e-3, r - 2e-3
    assert abs(P.rms_ratio(got[:3], model[:3], r[:3]) - 2.0) < 1e-9 and P.rms_ratio(model[:3], model[:3], r[:3]) == 1.0
    b = P.accum_budget(torch.tensor([1.0]), torch.tensor([10.0]), 100, torch.bfloat16)
    assert abs(float(b) - (2.0 ** -8 * (1 + 2.0 ** -10) + 2 * 100 * 2.0 ** -24 * 10)) < 1e-15
    assert float(P.truncate(torch.tensor([1.999, -1.999]), torch.bfloat16)[0]) == 1.9921875


# ---- family A ---------------------------------------------------------------------------------------------------------------------
def accum_figures(got, c, dtype):
    return (P.budget_fraction(got, c.r, P.accum_budget(c.r, c.sabs, c.terms, dtype)),
            P.misrounded_share(got, c.r, dtype) if dtype != torch.float32 else 0.0)


def model_meets_accum(c, dtype, share_cap=G.SHARE_CAP):
    frac, share = accum_figures(c.model, c, dtype)
    assert frac <= 1.0 and share <= ROOM * share_cap, (frac, share)
    assert P.rms_ratio(c.model, c.model, c.r) == 1.0
    return frac, share


@pytest.mark.parametrize("dtype", G.DTYPES, ids=G.IDS)
def test_family_a_models_keep_room(dtype):
    worst = [0.0, 0.0]
    cases = [G.gemm_case(dtype, M, N, K, epi) for M, N, K in G.GEMM_SHAPES for epi in G.GEMM_EPILOGUES]
    cases.append(G.gemm_case(dtype, *G.GEMM_TRANSPOSE[:3], "bias"))
    cases += [G.ln_gemm_case(dtype, M, N, K) for M, N, K in G.LN_GEMM_SHAPES]
    cases += [G.conv_case(dtype, Cin, Cout, mode) for Cin, Cout in G.CONV_CHANNELS for mode in ("s1", "s2", "up")]
    for c in cases:
        frac, share = model_meets_accum(c, dtype)
        worst = [max(worst[0], frac), max(worst[1], share)]
    if dtype == torch.float32:
        assert worst[0] <= 0.25          # f32: the model uses a small part of the budget (the issue measured <= 11 % on its inputs)
    for alpha in G.ADD_ALPHAS:
        c = G.add_case(dtype, alpha)
        assert (dtype == torch.float32 or P.misrounded_share(c.model, c.r, dtype) == 0.0) and accum_figures(c.model, c, dtype)[0] <= 1.0
    c = G.accumulate_case(dtype)
    assert P.misrounded_share(c.model, c.r, torch.float32) == 0.0


def gemm_mutants(b, dtype):
    """the GEMM with bias and residual, wrong in the ways a kernel change would be: each output has one or two roundings too many"""
    rd = lambda t: t.to(dtype).float()
    K = b.a.shape[1]
    h = K // 2
    split = rd(b.a[:, :h] @ b.w[:, :h].t()) + rd(b.a[:, h:] @ b.w[:, h:].t()) + b.bias + b.res
    twice = rd(rd(b.y32) + b.bias) + b.res
    once = rd(b.y32 + b.bias) + b.res
    return {"split-K partials rounded": split.to(dtype), "product rounded before bias and before residual": twice.to(dtype),
            "one extra rounding": once.to(dtype)}


@pytest.mark.parametrize("dtype", G.HALVES, ids=G.IDS)
@pytest.mark.parametrize("M,N,K", G.GEMM_SHAPES)
def test_family_a_mutants_fail_the_gate_and_pass_the_old_tolerance(dtype, M, N, K):
    c = G.gemm_case(dtype, M, N, K, "bias_res")
    for name, got in gemm_mutants(G.gemm_operands(dtype, M, N, K), dtype).items():
        frac, share = accum_figures(got, c, dtype)
        assert share >= 0.2 and share > G.SHARE_CAP, (name, share)
        assert passes_old_tol(got, c.r, dtype), name
    # the other legitimate order - one flat f32 sum over K, torch's own matmul - is inside the gate as well
    b = G.gemm_operands(dtype, M, N, K)
    frac, share = accum_figures((b.a @ b.w.t() + b.bias + b.res).to(dtype), c, dtype)
    assert frac <= 1.0 and share <= 0.5 * G.SHARE_CAP, (frac, share)


def test_staged_epilogue_model_and_its_mutants():
    """The two-rounding condition the GPU file keeps for the strictly-xfailed cases: the CPU model of the staged epilogue (product +
    bias rounded, residual / scale, rounded again) is inside staged_budget and OUTSIDE the one-rounding gate; one more rounding - the
    split-K partials rounded on top - fails the 1.12 rms cap against it"""
    for dtype, M, N, K, epi, _tile in G.staged_rows():
        c = G.gemm_case(dtype, M, N, K, epi)
        assert P.budget_fraction(c.model_staged, c.r, P.staged_budget(c.r, c.pre, c.scale, c.sabs, c.terms, dtype)) <= 1.0
        assert P.misrounded_share(c.model_staged, c.r, dtype) > G.SHARE_CAP
        if epi == "bias_res":
            b = G.gemm_operands(dtype, M, N, K)
            rd = lambda t: t.to(dtype).float()
            h = K // 2
            third = rd(rd(b.a[:, :h] @ b.w[:, :h].t()) + rd(b.a[:, h:] @ b.w[:, h:].t()) + b.bias) + b.res
            assert P.rms_ratio(third.to(dtype), c.model_staged, c.r) > G.RMS_CAP_C


def test_cases_reach_the_launches_named():
    """What the GPU file's cases launch, asked of the library without a GPU (emo_gemm_plan, emo_attention_plan,
    emo_groupnorm_one_launch_ok; the temporal dispatch mirrored): a later planner change cannot silently empty a case."""
    from emote_hack_amd import ops as o
    for dtype in G.DTYPES:
        for M, N, K in G.GEMM_SHAPES:
            for epi in G.GEMM_EPILOGUES:
                pl = o.gemm_plan(**G.gemm_plan_kw(G.gemm_case(dtype, M, N, K, epi), dtype, M, N, K, split_k=1))
                assert pl[0] == 0 and pl[4] == 1, pl
                if G.staged_twice(dtype, epi):
                    assert o.GEMM_STORE_PATHS[pl[5]] == "lds", (dtype, M, N, K, epi, pl)
        M, N, K = G.GEMM_SHAPES[0]
        c = G.gemm_case(dtype, M, N, K, "bias_res")
        seen = set()
        for t in G.GEMM_TILES[dtype]:
            pl = o.gemm_plan(**G.gemm_plan_kw(c, dtype, M, N, K, tile=t, split_k=1))
            assert t == 0 or pl[1] == t, (dtype, t, pl)                 # the plan admits the hint: this instantiation runs
            assert dtype == torch.float32 or o.GEMM_STORE_PATHS[pl[5]] == "lds", (dtype, t, pl)
            seen.add(pl[1])
        assert len(seen) == len(G.GEMM_TILES[dtype]) - 1                # (0 is the planner's choice of one of them)
        for t in range(8):                                              # ... and the table leaves out no tile the plan would admit
            if t not in G.GEMM_TILES[dtype]:
                assert o.gemm_plan(**G.gemm_plan_kw(c, dtype, M, N, K, tile=t, split_k=1))[1] != t
        M, N, K = G.GEMM_SHAPES[1]
        c = G.gemm_case(dtype, M, N, K, "bias_res")
        for sk in G.GEMM_SPLITS:
            pl = o.gemm_plan(**G.gemm_plan_kw(c, dtype, M, N, K, split_k=sk))
            assert pl[4] == sk and o.GEMM_STORE_PATHS[pl[5]] == "splitk_ws", pl
        M, N, K, L = G.GEMM_TRANSPOSE
        pl = o.gemm_plan(**G.gemm_plan_kw(G.gemm_case(dtype, M, N, K, "bias"), dtype, M, N, K, transpose_rows=L, transpose_ld=L, split_k=1))
        assert pl[3] & 2, pl
        for M, N, K in G.LN_GEMM_SHAPES:
            pl = o.gemm_plan(dtype=dtype, M=M, N=N, K=K, bias=True, ln=True)
            assert pl[3] & 4 and pl[4] == 1, pl
        for Cin, Cout in G.CONV_CHANNELS:
            for mode, path in G.CONV_RUNS:
                fam, flags = G.conv_plan_family(dtype, Cin, Cout, mode, path)
                assert (fam == 1) == path.startswith("halo") and (fam == 1 or flags & 1), (mode, path, fam, flags)
        for name, (B, heads, Lq, Lk0, Lk1, d) in G.ATTN_CASES.items():
            pl = o.attention_plan(dtype=dtype, B=B, Lq=Lq, Lk0=Lk0, heads=heads, d=d, Lk1=Lk1)
            assert (pl[3] > 1) == (name == "resident"), (name, pl)
        for shape in G.GN_ONE_LAUNCH_SHAPES:
            assert G.gn_one_launch_ok(dtype, *shape)
        for Fr, d in G.TEMPORAL_MFMA:
            assert G.temporal_takes_mfma(dtype, Fr, d) == (dtype != torch.float32)
        assert not G.temporal_takes_mfma(dtype, *G.TEMPORAL_GENERIC)


# ---- family B ---------------------------------------------------------------------------------------------------------------------
def family_b_cases(dtype):
    out = [G.ln_case(dtype, M, C) for M, C in G.LN_SHAPES]
    out += [G.gn_case(dtype, N, S, C, Gr, silu) for N, S, C, Gr in G.GN_SHAPES + G.GN_ONE_LAUNCH_SHAPES for silu in (False, True)]
    out += [G.gn_case(dtype, *G.GN_ONE_LAUNCH_SHAPES[0], True, kind, rows) for kind, rows in G.GN_MOD_CASES]
    out += [G.cn_case(dtype)]
    out += [G.softmax_case(dtype, M, N, s) for M, N, s in G.SOFTMAX_SHAPES]
    return out


@pytest.mark.parametrize("dtype", G.HALVES, ids=G.IDS)
def test_family_b_models_keep_room(dtype):
    for c in family_b_cases(dtype):
        share = P.misrounded_share(c.model, c.r, dtype)
        assert share <= ROOM * G.SHARE_CAP, share


def test_family_b_f32_models_are_f32_accurate():
    """the f32 condition is a ratio to the model's error: the model must be an f32 computation, not something coarser"""
    for c in family_b_cases(torch.float32):
        err = float(((c.model.double() - c.r).abs() / (c.r.abs() + 1.0)).max())
        assert 0 < err < 2e-5, err        # (a few f32 roundings of values 8 standard deviations from zero: 8 x a few x 2^-24)
        assert P.rms_ratio(c.model, c.model, c.r) == 1.0


@pytest.mark.parametrize("dtype", G.HALVES, ids=G.IDS)
def test_family_b_mutants_fail_the_gate_and_pass_the_old_tolerance(dtype):
    rd = lambda t: t.to(dtype).float()
    M, C = G.LN_SHAPES[0]
    c = G.ln_case(dtype, M, C)
    mean, var = c.x.mean(1, keepdim=True), c.x.var(1, unbiased=False, keepdim=True)
    muts = {"LayerNorm mean rounded": ((c.x - rd(mean)) / torch.sqrt(var + 1e-5) * c.gamma + c.beta, c),
            "LayerNorm normalised value rounded before the affine": (rd((c.x - mean) / torch.sqrt(var + 1e-5)) * c.gamma + c.beta, c)}
    N, S, Cc, Gr = G.GN_SHAPES[0]
    cg = G.gn_case(dtype, N, S, Cc, Gr, True)
    pre = rd(G.gn_math(cg.x, N, S, Cc, Gr, cg.gamma, cg.beta, 1e-5, False, None, 0))
    muts["GroupNorm rounded before the SiLU"] = (pre * torch.sigmoid(pre), cg)
    for name, (y, case) in muts.items():
        got = y.to(dtype)
        share = P.misrounded_share(got, case.r, dtype)
        assert share >= 0.1 and share > G.SHARE_CAP, (name, share)
        assert passes_old_tol(got, case.r, dtype), name


# ---- family C ---------------------------------------------------------------------------------------------------------------------
def heads_of(c, name):
    B, heads, Lq, Lk0, Lk1, d = G.ATTN_CASES[name]
    sp = lambda t: t.reshape(B, -1, heads, d).permute(0, 2, 1, 3)
    k, v = (c.k0, c.v0) if not Lk1 else (torch.cat([c.k0, c.k1], 1), torch.cat([c.v0, c.v1], 1))
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B * Lq, heads * d)
    return sp(c.q), sp(k), sp(v), back


def attention_variants(qh, kh, vh, scale, dtype):
    """(legitimate forms of the contract, mutants) as f32 computations of softmax(q k^T scale) v"""
    rd = lambda t: t.to(dtype).float()
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    e = torch.exp(s - s.amax(-1, keepdim=True))
    p = e / e.sum(-1, keepdim=True)
    half = vh.shape[-2] // 2
    legit = {"flash: unnormalised p rounded, row sum in f32": torch.matmul(rd(e), vh) / e.sum(-1, keepdim=True),
             "flash: unnormalised p rounded, row sum of the rounded p": torch.matmul(rd(e), vh) / rd(e).sum(-1, keepdim=True),
             "flash: reference 2^8 below the maximum": torch.matmul(rd(e * 256.0), vh) / rd(e * 256.0).sum(-1, keepdim=True)}
    mut = {"scores rounded before the softmax": torch.matmul(rd(torch.softmax(rd(s), -1)), vh),
           "output accumulated in two rounded halves": rd(torch.matmul(rd(p[..., :half]), vh[..., :half, :])) + rd(torch.matmul(rd(p[..., half:]), vh[..., half:, :])),
           "P truncated": torch.matmul(P.truncate(p, dtype), vh)}
    return legit, mut


@pytest.mark.parametrize("dtype", G.DTYPES, ids=G.IDS)
def test_family_c_models_keep_room(dtype):
    cases = [G.attn_case(dtype, n) for n in G.ATTN_CASES] + [G.temporal_case(dtype, Fr, d) for Fr, d in G.TEMPORAL_MFMA + [G.TEMPORAL_GENERIC]]
    for c in cases:
        frac = P.budget_fraction(c.model, c.r, P.attention_budget(c.r, c.pabsv, c.L, c.d, c.vmax, dtype))
        assert frac <= 1.0, frac
        assert P.rms_ratio(c.model, c.model, c.r) == 1.0


@pytest.mark.parametrize("dtype", G.HALVES, ids=G.IDS)
@pytest.mark.parametrize("name", ["single_150_d40", "single_77_d160", "single_12_d40"])
def test_family_c_forms_and_mutants(dtype, name):
    c = G.attn_case(dtype, name)
    qh, kh, vh, back = heads_of(c, name)
    legit, mut = attention_variants(qh, kh, vh, c.scale, dtype)
    budget = P.attention_budget(c.r, c.pabsv, c.L, c.d, c.vmax, dtype)
    for form, y in legit.items():
        got = back(y).to(dtype)
        ratio = P.rms_ratio(got, c.model, c.r)
        assert ratio <= 1.05 and P.budget_fraction(got, c.r, budget) <= 1.0, (form, ratio)
    for form, y in mut.items():
        got = back(y).to(dtype)
        ratio = P.rms_ratio(got, c.model, c.r)
        assert ratio >= 1.2 and ratio > G.RMS_CAP_C, (form, ratio)
        assert passes_old_tol(got, c.r, dtype), form


# ---- family D ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", G.HALVES, ids=G.IDS)
@pytest.mark.parametrize("kind", G.ACT_KINDS)
def test_family_d_models_keep_room(dtype, kind):
    """torch's own f32 activations over every 16-bit input meet the budget of the kernels' claims and a quarter of the share cap;
    the limits at the infinities are what the GPU file asks for, wherever f32 arithmetic can give them"""
    c = G.act_case(dtype, kind)
    fin = c.finite
    r, m = c.r[fin], c.model.double()[fin]
    budget = 0.5 * P.ulp(r, dtype) * (1 + 2.0 ** -10) + G.act_allowance(c.x[fin], r, kind)
    assert bool(((m - r).abs() <= budget).all())
    assert P.misrounded_share(m, r, dtype) <= ROOM * G.SHARE_CAP
    assert c.x.numel() == 65536 and int(torch.isnan(c.x).sum()) == (254 if dtype == torch.bfloat16 else 2046)
    assert G.act_math(torch.tensor([float("inf"), -float("inf")]), kind).tolist() == {"tanh": [1.0, -1.0]}.get(kind, [float("inf"), 0.0])


@pytest.mark.parametrize("dtype", G.HALVES, ids=G.IDS)
def test_family_d_mutants_fail_the_gate(dtype):
    """a coarser transcendental - the sigmoid's exponential through the two-byte type - fails share and budget; the GEGLU reference
    with an error of TWICE the claimed 1.9e-4 fails the GEGLU budget, with the claimed error it passes"""
    c = G.act_case(dtype, "silu")
    fin = c.finite
    x = c.x[fin]
    got = (x / (1 + torch.exp(-x).to(dtype).float())).to(dtype).double()
    budget = 0.5 * P.ulp(c.r[fin], dtype) * (1 + 2.0 ** -10) + G.act_allowance(x, c.r[fin], "silu")
    assert P.misrounded_share(got, c.r[fin], dtype) > 0.5 * G.SHARE_CAP and not bool(((got - c.r[fin]).abs() <= budget).all())
    g = G.geglu_case(dtype)
    ok = torch.isfinite(g.g) & (g.g.abs() < 4)
    budget = 0.5 * P.ulp(g.r, dtype) + g.v.abs() * G.GEGLU_CLAIM * (1 + 2.0 ** -6)
    for k, passes in ((0.9, True), (2.0, False)):
        got = P.correctly_rounded(g.r + k * G.GEGLU_CLAIM * g.v, dtype).double()
        assert bool(((got - g.r).abs()[ok] <= budget[ok]).all()) == passes
