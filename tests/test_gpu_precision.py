"""The precision gate of the kernel suite: every arithmetic kernel against an f64 statement of the same operation on the same
(quantised) inputs, held to a bound DERIVED from its rounding contract (tests/precision_ref.py) - not to the blanket TOL of
tests/test_gpu_kernels.py, which lets a third of all outputs be wrong in the last place (tests/test_precision_ref_host.py shows it:
every mutant listed there passes TOL and fails the condition of its family here).  No figure of a kernel sets a condition: the caps
come from the CPU models of the contracts, which the host file holds to a quarter of each cap on the inputs built below.

Rounding contracts (DESIGN.md "Rounding contract"):

  operation                    inner roundings                                                     where the code says so
  ---------------------------  ------------------------------------------------------------------  ------------------------------
  gemm / conv3x3 (family A)    none: f32 accumulate (MFMA), f32 epilogue, ONE output rounding;     gemm_impl.h epilogue_*; split-K
                               split-K partials stay f32                                           workspace: emo_hip.h split_k
  add / accumulate_window      none: one f32 operation, one rounding                               elementwise.hip add_kernel
  norms / softmax (family B)   none: f32 statistics, f32 normalise + affine (+ SiLU), one rounding  norm.hip, frontend.hip
  attention (family C)         P rounded to the dtype: UNNORMALISED p = exp2(s - m_run) (<= 2^8),   attention.hip:456-505 (pack2),
                               P.V and the row sum accumulate in f32 - the row sum of the ROUNDED   attention.hip:165,487,605
                               p where the head dim leaves a pad row (d = 40, 80), of the f32 p
                               otherwise (d = 160) -, one division, one output rounding
                               (the TESTED model rounds the normalised P; the flash forms are held
                               to <= 1.05 of it on the CPU, so the same 1.12 covers the kernel)
  temporal_attention (C)       NORMALISED p rounded to the dtype, P.V in f32, one output rounding   temporal.hip:102-114, 255-275
  silu / act (family D)        none: f32 transcendental, one rounding                              common.h:180-197
  GEGLU epilogue (family D)    none; gelu by polynomial, |error| <= 1.9e-4 absolute                common.h:198-220

Measured on an MI355X (worst over the cases of each table; budget = max |got - r| / budget, share = misrounded share,
rms = rms_ratio against the CPU model): see the comment at each case table.

Every test prints its figures ("PREC ...") before it asserts."""
import functools
import math
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn.functional as F

from tests import precision_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
HALVES = [torch.bfloat16, torch.float16]
IDS = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}.get
SHARE_CAP = 0.01          # families A, B, D: two-byte outputs that are not the correctly rounded exact value
RMS_CAP_F32 = 4.0         # family B, f32: rms error against the CPU f32 model's
RMS_CAP_C = 1.12          # family C: rms error against the CPU model of the contract (legitimate forms <= 1.00, mutants >= 1.24)


def ops():
    from emote_hack_amd import ops as o
    return o


def q(t, dtype):
    return t.to(dtype).float()


def dev(t, dtype):
    return t.to(DEV).to(dtype)


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def f32c(v):
    """a Python float as the kernel sees it: through a C float"""
    return float(torch.tensor(v, dtype=torch.float32))


def report(label, **figs):
    print("PREC " + label + " " + " ".join(f"{k}={v:.4g}" for k, v in figs.items()))


def check_accum(label, got, c, dtype, share_cap=SHARE_CAP):
    """family A: |got - r| <= accum_budget everywhere; two-byte types: misrounded share <= share_cap"""
    frac = P.budget_fraction(got, c.r, P.accum_budget(c.r, c.sabs, c.terms, dtype))
    share = P.misrounded_share(got, c.r, dtype) if dtype != torch.float32 or share_cap == 0 else float("nan")
    report(label, budget=frac, share=share)
    assert frac <= 1.0, f"{label}: {frac:.3f} of the accumulation budget"
    if share == share:
        assert share <= share_cap, f"{label}: misrounded share {share:.4f} > {share_cap}"
    return frac, share


def check_rounded(label, got, c, dtype):
    """family B: two-byte types: misrounded share <= SHARE_CAP; f32: rms error <= RMS_CAP_F32 x the CPU f32 model's"""
    if dtype == torch.float32:
        ratio = P.rms_ratio(got, c.model, c.r)
        report(label, rms=ratio)
        assert ratio <= RMS_CAP_F32, f"{label}: rms error {ratio:.2f} x the f32 model's"
        return ratio
    share = P.misrounded_share(got, c.r, dtype)
    report(label, share=share)
    assert share <= SHARE_CAP, f"{label}: misrounded share {share:.4f} > {SHARE_CAP}"
    return share


# =================================================================================================== family A: dense GEMM
# (M, N, K) / epilogue / tile / split / store tables of the dense GEMM; measured figures below GEMM_STAGED_EPILOGUES
GEMM_SHAPES = [(257, 320, 320), (130, 96, 2560), (64, 64, 24)]          # (M, N, K): ragged M, long K, one short K step
GEMM_EPILOGUES = ["none", "bias", "bias_res", "scale", "rowbias"]
GEMM_RPB = {257: 64, 130: 64, 64: 16, 256: 64}                            # rows per row-bias batch
# emo_gemm_params.tile hints the plan admits at (257, 320, 320) with bias + residual (0 = the planner's own choice; f32 has no 256x320 / phase-loop tile)
GEMM_TILES = {torch.float32: list(range(6)), torch.bfloat16: list(range(8)), torch.float16: list(range(8))}
# OPEN FINDING: the LDS-staged epilogue of the two-byte types (gemm_impl.h epilogue_lds) packs product + bias + row bias to the dtype
# for the transpose through LDS (phase 1), unpacks, adds the residual and scales (phase 2: RES = residual or out_scale != 1) and rounds
# AGAIN - "one extra rounding".  Measured: 28-30 % of the outputs misrounded at every shape and tile, up to 120 x the budget at K = 24.
# Staging f32 instead would double the epilogue's LDS traffic on the flagship GEMMs: not changed without a timing; the cases stay,
# strictly expected to fail, until the epilogue adds the residual before its one rounding.
GEMM_STAGED_EPILOGUES = ("bias_res", "scale")
STAGED_XFAIL = pytest.mark.xfail(strict=True, raises=AssertionError, reason="two-byte LDS-staged epilogue rounds before the residual / scale pass and again after it "
                                                     "(gemm_impl.h epilogue_lds): 28-30 % of the outputs misrounded")
GEMM_SPLITS = [2, 5]                                                      # at (130, 96, 2560)
GEMM_TRANSPOSE = (256, 64, 64, 64)                                        # (M, N, K, L)
OUT_SCALE = 0.3                                                           # not a power of two: the scaling is an f32 operation
# measured (MI355X), worst over the cases that round once - epilogues none / bias / rowbias, split-K 2 and 5 with bias + residual, V^T:
#   f32   budget <= 0.054 (every epilogue, every tile)
#   bf16  budget <= 0.997, share <= 4.8e-4   (split-K 0.60 / 1.6e-4, V^T 0.993 / 0)
#   f16   budget <= 0.985, share <= 1.8e-3   (the long-K shape: 1.6e-3 to 1.8e-3, inside the cap; split-K 0.16 / 1.1e-3, V^T 0.959 / 4.9e-4)
# and over the strictly-xfailed cases - bias + residual, out_scale, every tile hint: share 0.283 to 0.295, budget up to 120.6 (bf16) / 29.8 (f16)


def matmul32(a, w):
    """a @ w.T in f32 with K summed in chunks of 32, the chunks added in order: the f32-accumulate MODEL of an MFMA main loop (one
    flat f32 sum over K = 2560 misrounds 3e-3 of the f16 outputs by itself; the kernels' order is closer to this one)"""
    return sum((a[:, k:k + 32] @ w[:, k:k + 32].t() for k in range(0, a.shape[1], 32)), torch.zeros(a.shape[0], w.shape[0]))


@functools.lru_cache(maxsize=None)
def gemm_operands(dtype, M, N, K):
    g = gen(7927 * M + 31 * N + K)
    a = q(torch.randn(M, K, generator=g), dtype)
    w = q(torch.randn(N, K, generator=g) / math.sqrt(K), dtype)
    bias = 0.1 * torch.randn(N, generator=g)
    rpb = GEMM_RPB[M]
    rb = torch.randn((M + rpb - 1) // rpb, N, generator=g)
    res = q(torch.randn(M, N, generator=g), dtype)
    return NS(a=a, w=w, bias=bias, rb=rb, rpb=rpb, res=res, y64=a.double() @ w.double().t(), yabs=a.double().abs() @ w.double().abs().t(),
              y32=matmul32(a, w))


def gemm_case(dtype, M, N, K, epi):
    """operands, f64 value r, the same on absolute values, the f32 operation count and the CPU f32 model of one dense GEMM"""
    b = gemm_operands(dtype, M, N, K)
    c = NS(a=b.a, w=b.w, bias=None, rb=None, rpb=0, res=None, scale=1.0, terms=K + 4)
    r, sabs, m = b.y64, b.yabs, b.y32
    if epi in ("bias", "bias_res", "scale", "rowbias"):
        c.bias = b.bias
        r, sabs, m = r + b.bias.double(), sabs + b.bias.double().abs(), m + b.bias
    if epi == "rowbias":
        c.rb, c.rpb = b.rb, b.rpb
        rows = b.rb[torch.arange(M) // b.rpb]
        r, sabs, m = r + rows.double(), sabs + rows.double().abs(), m + rows
    c.pre, m2 = r, m.to(dtype).float()          # what the LDS-staged epilogue packs to the dtype before its residual / scale pass
    if epi == "bias_res":
        c.res = b.res
        r, sabs, m, m2 = r + b.res.double(), sabs + b.res.double().abs(), m + b.res, m2 + b.res
    if epi == "scale":
        c.scale = f32c(OUT_SCALE)
        r, sabs, m, m2 = r * c.scale, sabs * c.scale, m * torch.tensor(c.scale, dtype=torch.float32), m2 * torch.tensor(c.scale, dtype=torch.float32)
    c.r, c.sabs, c.model, c.model_staged = r, sabs, m.to(dtype), m2.to(dtype)
    return c


def gemm_plan_kw(c, dtype, M, N, K, **kw):
    return dict(dtype=dtype, M=M, N=N, K=K, bias=c.bias is not None, rowbias=c.rb is not None, rows_per_batch=c.rpb,
                residual=c.res is not None, out_scale=c.scale, **kw)


def run_gemm(c, dtype, **kw):
    o = ops()
    return o.gemm(dev(c.a, dtype), dev(c.w, dtype).contiguous(), None if c.bias is None else c.bias.to(DEV),
                  rowbias=None if c.rb is None else c.rb.to(DEV), rows_per_batch=c.rpb, residual=None if c.res is None else dev(c.res, dtype),
                  out_scale=c.scale, **kw).float().cpu()


def staged_twice(dtype, epi):
    return dtype != torch.float32 and epi in GEMM_STAGED_EPILOGUES


def gemm_params(rows):
    """pytest params of (dtype, ..., epilogue) rows; the cases of GEMM_STAGED_EPILOGUES in the two-byte types carry the strict xfail"""
    return [pytest.param(*row, marks=[STAGED_XFAIL] if staged_twice(row[0], row[-1]) else [],
                         id="-".join([IDS(row[0])] + [str(v) for v in row[1:]])) for row in rows]


def staged_rows():
    """(dtype, M, N, K, epilogue, tile hint) of every strictly-xfailed case"""
    M0, N0, K0 = GEMM_SHAPES[0]
    return [(dt_, M, N, K, epi, 0) for dt_ in HALVES for M, N, K in GEMM_SHAPES for epi in GEMM_STAGED_EPILOGUES] + \
           [(dt_, M0, N0, K0, "bias_res", t) for dt_ in HALVES for t in GEMM_TILES[dt_] if t]


# (what each case launches - single pass, the tile asked for, the LDS store path of the marked cases - is asserted on the CPU:
# tests/test_precision_ref_host.py test_cases_reach_the_launches_named; the xfailed bodies hold the precision condition alone)
@pytest.mark.parametrize("dtype,M,N,K,epi", gemm_params([(dt_, M, N, K, epi) for dt_ in DTYPES for M, N, K in GEMM_SHAPES for epi in GEMM_EPILOGUES]))
def test_gemm_epilogues_round_once(dtype, M, N, K, epi):
    """Dense GEMM, every epilogue, single pass: f32 accumulate, one rounding.  The long-K shape alone may exceed the share cap while
    inside the budget (the MFMA accumulate itself) - it does not: the cap holds for it as well."""
    c = gemm_case(dtype, M, N, K, epi)
    got = run_gemm(c, dtype, split_k=1)
    check_accum(f"gemm {IDS(dtype)} {M}x{N}x{K} {epi}", got, c, dtype)


@pytest.mark.parametrize("dtype,tile,epi", gemm_params([(dt_, t, "bias_res") for dt_ in DTYPES for t in GEMM_TILES[dt_]]))
def test_gemm_every_admitted_tile_rounds_once(dtype, tile, epi):
    M, N, K = GEMM_SHAPES[0]
    c = gemm_case(dtype, M, N, K, epi)
    got = run_gemm(c, dtype, split_k=1, tile=tile)
    check_accum(f"gemm {IDS(dtype)} tile={tile} {epi}", got, c, dtype)


@pytest.mark.parametrize("dtype,M,N,K,epi,tile", [pytest.param(*row, id="-".join([IDS(row[0])] + [str(v) for v in row[1:]])) for row in staged_rows()])
def test_gemm_staged_epilogue_rounds_twice_and_no_more(dtype, M, N, K, epi, tile):
    """The cases the strict xfails above leave open are still held: to the budget of the two roundings the staged epilogue documents
    (half an ulp of product + bias where it is packed for LDS, scaled as the value is afterwards; half an ulp of the output; the f32
    terms) and to 1.12 x the rms error of the CPU model with exactly that extra rounding - a third rounding, a lowered accumulator
    or a dropped term in the residual pass fails here.    measured: budget <= 0.995 (bf16) / 0.988 (f16), rms ratio 1.000 to 1.001 on every shape and tile"""
    c = gemm_case(dtype, M, N, K, epi)
    got = run_gemm(c, dtype, split_k=1, tile=tile)
    frac = P.budget_fraction(got, c.r, P.staged_budget(c.r, c.pre, c.scale, c.sabs, c.terms, dtype))
    ratio = P.rms_ratio(got, c.model_staged, c.r)
    report(f"gemm staged {IDS(dtype)} {M}x{N}x{K} {epi} tile={tile}", budget=frac, rms=ratio)
    assert frac <= 1.0, frac
    assert ratio <= RMS_CAP_C, ratio


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("sk", GEMM_SPLITS)
def test_gemm_split_k_workspace_costs_no_rounding(dtype, sk):
    o = ops()
    M, N, K = GEMM_SHAPES[1]
    c = gemm_case(dtype, M, N, K, "bias_res")
    pl = o.gemm_plan(**gemm_plan_kw(c, dtype, M, N, K, split_k=sk))
    assert pl[4] == sk and o.GEMM_STORE_PATHS[pl[5]] == "splitk_ws", pl
    check_accum(f"gemm {IDS(dtype)} {M}x{N}x{K} split_k={sk} bias_res", run_gemm(c, dtype, split_k=sk), c, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gemm_transposed_store_rounds_once(dtype):
    o = ops()
    M, N, K, L = GEMM_TRANSPOSE
    c = gemm_case(dtype, M, N, K, "bias")
    pl = o.gemm_plan(**gemm_plan_kw(c, dtype, M, N, K, transpose_rows=L, transpose_ld=L, split_k=1))
    assert pl[3] & 2, pl                                       # the V^T kernel
    got = run_gemm(c, dtype, split_k=1, transpose_rows=L, transpose_ld=L)
    check_accum(f"gemm {IDS(dtype)} {M}x{N}x{K} V^T L={L} bias", got.permute(0, 2, 1).reshape(M, N), c, dtype)


# ---- LayerNorm folded into the GEMM: the reference is f64 on the PACKED operands (rounded folded weights, f32 column sums and
# bias), LayerNorm statistics in f64.  terms: K for the product, K for the f32 column sums the correction multiplies, K for the f32
# statistics, 16 for the epilogue; sabs counts the correction with sum |w|, which is what an error of the column sums scales with.
# measured: f32 budget <= 0.014; bf16 budget <= 0.986, share <= 4.0e-4; f16 budget <= 0.946, share <= 1.5e-3
LN_GEMM_SHAPES = [(257, 320, 320), (130, 96, 1280), (64, 64, 24)]        # K = 1280: the widest LayerNorm of the model (and the widest the f32 kernel serves)
LN_ROW_OFFSET = 0.5        # spread of the row means: with 1.5, as the sweeps use, the f32 MODEL's own misrounded share in f16 at K = 2560
                           # is 3e-3 to 4e-3 - the cancellation against mean * colsum costs f32 bits - and keeps no room under the cap


@functools.lru_cache(maxsize=None)
def ln_gemm_case(dtype, M, N, K):
    g = gen(4001 + 7 * N + K)
    a = q(torch.randn(M, K, generator=g) * 1.3 + LN_ROW_OFFSET * torch.randn(M, 1, generator=g), dtype)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = 0.1 * torch.randn(N, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    wp = (w * gamma[None, :]).to(dtype)                        # what unet._pack does (tests/test_gpu_gemm_sweeps.py ln_fold)
    bp = w.to(dtype).float() @ beta + bias
    cs = wp.float().sum(1)
    a64, w64 = a.double(), wp.double()
    mean, var = a64.mean(1, keepdim=True), a64.var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    r = ((a64 - mean) * rstd) @ w64.t() + bp.double()
    sabs = rstd * (a64.abs() @ w64.abs().t() + mean.abs() * w64.abs().sum(1)[None, :]) + bp.double().abs()
    mean32, var32 = a.mean(1, keepdim=True), a.var(1, unbiased=False, keepdim=True)
    rstd32 = 1.0 / torch.sqrt(var32 + 1e-5)
    model = (rstd32 * (matmul32(a, wp.float()) - mean32 * cs[None, :]) + bp).to(dtype)
    return NS(a=a, wp=wp, bp=bp, cs=cs, r=r, sabs=sabs, terms=3 * K + 16, model=model)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,N,K", LN_GEMM_SHAPES)
def test_gemm_layernorm_fold_rounds_once(dtype, M, N, K):
    o = ops()
    c = ln_gemm_case(dtype, M, N, K)
    pl = o.gemm_plan(dtype=dtype, M=M, N=N, K=K, bias=True, ln=True)
    assert pl[3] & 4 and pl[4] == 1, pl
    ad = dev(c.a, dtype)
    got = o.gemm(ad, c.wp.to(DEV).contiguous(), c.bp.to(DEV), ln=(c.cs.to(DEV), o.layer_norm_stats(ad, 1e-5))).float().cpu()
    check_accum(f"gemm+ln {IDS(dtype)} {M}x{N}x{K}", got, c, dtype)


# =================================================================================================== family A: 3x3 conv
# n = 2 frames of 16 x 16.  mode: s1 = stride 1, s2 = stride 2, up = nearest x2 upsampling in front of the conv.  path: the halo-reuse
# kernel on 8- / 16-row patches (tile bits 1 / 2, as tests/halo_sweep_cases.py pins them) or the im2col loader of the tile GEMM
# (stride 2 always; stride 1 and x2 under split_k = 2, which the halo kernel does not serve).  K = 9 Cin in the budget.
# measured: f32 budget <= 0.0044; bf16 budget <= 0.922, share <= 2.4e-4; f16 budget <= 0.649, share <= 1.2e-3 (no path stands out)
CONV_N, CONV_HW = 2, 16
CONV_CHANNELS = [(64, 64), (64, 132), (128, 320)]
CONV_RUNS = [("s1", "halo8"), ("s1", "halo16"), ("s1", "im2col"), ("s2", "im2col"), ("up", "halo8"), ("up", "halo16"), ("up", "im2col")]
CONV_PATH_KW = {"halo8": dict(split_k=1, tile=1), "halo16": dict(split_k=1, tile=2)}


def conv_path_kw(mode, path):
    return CONV_PATH_KW.get(path) or dict(split_k=1 if mode == "s2" else 2)


@functools.lru_cache(maxsize=None)
def conv_case(dtype, Cin, Cout, mode):
    g = gen(5003 + 3 * Cin + Cout)
    n, H = CONV_N, CONV_HW
    x = q(torch.randn(n, Cin, H, H, generator=g), dtype)
    wt = q(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin), dtype)
    bias = 0.1 * torch.randn(Cout, generator=g)
    stride = 2 if mode == "s2" else 1
    xi = F.interpolate(x, scale_factor=2.0, mode="nearest") if mode == "up" else x
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, Cout)
    r = rows(F.conv2d(xi.double(), wt.double(), bias.double(), stride=stride, padding=1))
    sabs = rows(F.conv2d(xi.abs(), wt.abs(), bias.abs(), stride=stride, padding=1)).double() * (1 + 1e-5)     # (a bound: f32 will do)
    model = rows(F.conv2d(xi, wt, bias, stride=stride, padding=1)).to(dtype)
    return NS(x=x.permute(0, 2, 3, 1).reshape(-1, Cin).contiguous(), w=wt.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous(), bias=bias,
              stride=stride, up=mode == "up", r=r, sabs=sabs, terms=9 * Cin + 4, model=model)


def conv_plan_family(dtype, Cin, Cout, mode, path):
    """(family, flags) of emo_gemm_plan for one conv run: family 1 = the halo-reuse kernel; flags bit 0 = the im2col loader"""
    o = ops()
    H = CONV_HW
    He = 2 * H if mode == "up" else H
    stride = 2 if mode == "s2" else 1
    Ho = (He + 2 - 3) // stride + 1
    pl = o.gemm_plan(dtype=dtype, M=CONV_N * Ho * Ho, N=Cout, K=9 * Cin, bias=True,
                     conv=dict(H=H, W=H, Cin=Cin, stride=stride, upsample2x=mode == "up", Ho=Ho, Wo=Ho), **conv_path_kw(mode, path))
    return pl[0], pl[3]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Cin,Cout", CONV_CHANNELS)
def test_conv3x3_rounds_once(dtype, Cin, Cout):
    o = ops()
    for mode, path in CONV_RUNS:
        fam, flags = conv_plan_family(dtype, Cin, Cout, mode, path)
        assert (fam == 1) == path.startswith("halo") and (fam == 1 or flags & 1), (mode, path, fam, flags)
        c = conv_case(dtype, Cin, Cout, mode)
        got, _, _ = o.conv3x3(dev(c.x, dtype), dev(c.w, dtype), c.bias.to(DEV), CONV_N, CONV_HW, CONV_HW, stride=c.stride, upsample2x=c.up,
                              **conv_path_kw(mode, path))
        check_accum(f"conv {IDS(dtype)} {Cin}->{Cout} {mode} {path}", got.float().cpu(), c, dtype)


# =================================================================================================== family A: one operation, one rounding
# alpha is a power of two times 1 or 3: a + alpha * b of two-byte operands is exact in f32, so the ONE rounding is the output's and
# the share must be 0; f32 (where 1.5 b rounds) gets the budget of its two operations.    measured: share 0, f32 budget 0.20
ADD_SHAPE, ADD_ALPHAS = (37, 24), [0.5, -1.5]


@functools.lru_cache(maxsize=None)
def add_case(dtype, alpha):
    g = gen(6007)
    a, b = q(torch.randn(ADD_SHAPE, generator=g), dtype), q(torch.randn(ADD_SHAPE, generator=g), dtype)
    r = a.double() + alpha * b.double()
    return NS(a=a, b=b, r=r, sabs=a.double().abs() + abs(alpha) * b.double().abs(), terms=2, model=(a + alpha * b).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_add_is_one_rounding(dtype):
    o = ops()
    for alpha in ADD_ALPHAS:
        c = add_case(dtype, alpha)
        got = o.add(dev(c.a, dtype), dev(c.b, dtype), alpha=alpha).float().cpu()
        check_accum(f"add {IDS(dtype)} alpha={alpha}", got, c, dtype, share_cap=0.0 if dtype != torch.float32 else SHARE_CAP)


ACC_GEOM = dict(C_=4, F=6, HW=20)
ACC_FRAMES = [4, 5, 0]


@functools.lru_cache(maxsize=None)
def accumulate_case(dtype):
    g = gen(6011)
    C4, Ft, HW = ACC_GEOM["C_"], ACC_GEOM["F"], ACC_GEOM["HW"]
    pred = q(torch.randn(len(ACC_FRAMES) * HW, C4, generator=g), dtype)
    start = torch.randn(C4, Ft, HW, generator=g)
    r, m = start.double().clone(), start.clone()
    upd = pred.reshape(len(ACC_FRAMES), HW, C4).permute(2, 0, 1)
    r[:, ACC_FRAMES] += upd.double()
    m[:, ACC_FRAMES] += upd
    return NS(pred=pred, start=start, r=r, model=m)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_accumulate_window_is_one_rounding(dtype):
    """the f32 accumulator += one row of any dtype: one f32 addition, so every element is the correctly rounded f32 sum"""
    o = ops()
    c = accumulate_case(dtype)
    acc, cnt = c.start.clone().to(DEV), torch.zeros(ACC_GEOM["F"], device=DEV)
    o.accumulate_window(dev(c.pred, dtype), acc, cnt, torch.tensor(ACC_FRAMES, dtype=torch.int32, device=DEV), add_counter=True, **ACC_GEOM)
    share = P.misrounded_share(acc.cpu(), c.r, torch.float32)
    report(f"accumulate_window {IDS(dtype)}", share=share)
    assert share == 0.0


# =================================================================================================== family B: norms and softmax
# measured (share, two-byte / rms ratio, f32):
#   layer_norm   bf16 <= 1.6e-4, f16 <= 5.3e-4, f32 rms 0.92
#   group_norm   bf16 <= 1.1e-3, f16 <= 3.8e-3, f32 rms 0.26 to 1.42   (one- and two-launch, SiLU, mod, mod_rows; the largest with mod)
#   channel_norm bf16 0,         f16 1.8e-4,    f32 rms 0.21
#   softmax_rows bf16 0,         f16 0,         f32 rms 1.04 to 1.22
LN_SHAPES = [(77, 320), (100, 64)]
GN_SHAPES = [(2, 100, 64, 8), (2, 256, 320, 32)]                          # (instances, rows per instance, C, groups): two launches
GN_ONE_LAUNCH_SHAPES = [(4, 100, 64, 8), (4, 256, 320, 32)]               # the same with the 32 blocks the one-launch kernel asks for
GN_OFFSET = 8.0                                                           # common offset in standard deviations
GN_MOD_CASES = [("mod", 0), ("mod_rows", 50)]                            # at GN_ONE_LAUNCH_SHAPES[0], SiLU on: per instance / per 50 rows
CN_SHAPE = (799, 96)
SOFTMAX_SHAPES = [(64, 77, 0.125), (35, 35, 1.0)]                         # (rows, columns, scale)


@functools.lru_cache(maxsize=None)
def ln_case(dtype, M, C):
    g = gen(7001 + C)
    x = q(torch.randn(M, C, generator=g) * 1.3 + 1.5 * torch.randn(M, 1, generator=g), dtype)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    return NS(x=x, gamma=gamma, beta=beta, r=F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5),
              model=F.layer_norm(x, (C,), gamma, beta, 1e-5).to(dtype))


def offset_rows(N, S, C, G, g, dtype, spread=2.0):
    """(N * S, C) rows whose N x G normalised units all have standard deviation `spread` and mean GN_OFFSET * spread (before the
    quantisation to dtype), as tests/test_gpu_kernels.py _offset_rows builds them"""
    z = torch.randn(N * S, C, generator=g).double().reshape(N, S, G, C // G)
    z = (z - z.mean((1, 3), keepdim=True)) / z.std((1, 3), unbiased=False, keepdim=True)
    return q((z * spread + GN_OFFSET * spread).float().reshape(N * S, C), dtype)


def gn_math(x, N, S, C, G, gamma, beta, eps, silu, mod, mod_rows):
    """GroupNorm (+ scale-shift modulation) (+ SiLU) in the dtype of x: f64 = the reference, f32 = the model"""
    u = x.reshape(N, S, G, C // G)
    mean, var = u.mean((1, 3), keepdim=True), u.var((1, 3), unbiased=False, keepdim=True)
    y = ((u - mean) / torch.sqrt(var + eps)).reshape(N * S, C) * gamma.to(x.dtype) + beta.to(x.dtype)
    if mod is not None:
        rows = mod.to(x.dtype).repeat_interleave(mod_rows or S, 0)
        y = y * (1 + rows[:, :C]) + rows[:, C:]
    return y * torch.sigmoid(y) if silu else y


@functools.lru_cache(maxsize=None)
def gn_case(dtype, N, S, C, G, silu, mod_kind=None, mod_rows=0):
    g = gen(7013 + C + (1 if mod_kind else 0))
    x = offset_rows(N, S, C, G, g, dtype)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    mod = None
    if mod_kind:
        mod = 0.3 * torch.randn(N * S // mod_rows if mod_rows else N, 2 * C, generator=g)
    return NS(x=x, gamma=gamma, beta=beta, mod=mod, mod_rows=mod_rows,
              r=gn_math(x.double(), N, S, C, G, gamma, beta, 1e-5, silu, mod, mod_rows),
              model=gn_math(x, N, S, C, G, gamma, beta, 1e-5, silu, mod, mod_rows).to(dtype))


@functools.lru_cache(maxsize=None)
def cn_case(dtype):
    S, C = CN_SHAPE
    g = gen(7019)
    x = offset_rows(1, S, C, C, g, dtype)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    return NS(x=x, gamma=gamma, beta=beta, r=gn_math(x.double(), 1, S, C, C, gamma, beta, 1e-5, False, None, 0),
              model=gn_math(x, 1, S, C, C, gamma, beta, 1e-5, False, None, 0).to(dtype))


@functools.lru_cache(maxsize=None)
def softmax_case(dtype, M, N, scale):
    x = q(torch.randn(M, N, generator=gen(7027 + N)) * 3, dtype)
    s = f32c(scale)
    return NS(x=x, scale=s, r=torch.softmax(x.double() * s, -1), model=torch.softmax(x * torch.tensor(s, dtype=torch.float32), -1).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,C", LN_SHAPES)
def test_layer_norm_rounds_once(dtype, M, C):
    o = ops()
    c = ln_case(dtype, M, C)
    got = o.layer_norm(dev(c.x, dtype), c.gamma.to(DEV), c.beta.to(DEV), 1e-5).float().cpu()
    check_rounded(f"layer_norm {IDS(dtype)} {M}x{C}", got, c, dtype)


def gn_one_launch_ok(dtype, N, S, C, G):
    from emote_hack_amd import _lib
    return _lib.load().emo_groupnorm_one_launch_ok(N, S, C, G, ops().dt(dtype)) == 1


def run_group_norm(c, dtype, N, G, silu, one_launch):
    o = ops()
    saved = o.GN_ONE_LAUNCH
    o.GN_ONE_LAUNCH = one_launch          # the A/B hook of ops.group_norm: False = the statistics + apply pair
    try:
        return o.group_norm(dev(c.x, dtype), c.gamma.to(DEV), c.beta.to(DEV), N, G, 1e-5, silu,
                            mod=None if c.mod is None else c.mod.to(DEV), mod_rows=c.mod_rows).float().cpu()
    finally:
        o.GN_ONE_LAUNCH = saved


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N,S,C,G", GN_SHAPES + GN_ONE_LAUNCH_SHAPES)
def test_group_norm_rounds_once(dtype, N, S, C, G):
    """the statistics + apply pair at every shape, the one-launch kernel where the library offers it (two instances are too few
    blocks for it in the two-byte types), SiLU on and off, inputs with a common offset of 8 standard deviations"""
    one_ok = gn_one_launch_ok(dtype, N, S, C, G)
    assert one_ok or (N, S, C, G) in GN_SHAPES
    for silu in (False, True):
        c = gn_case(dtype, N, S, C, G, silu)
        for one in ((True, False) if one_ok else (False,)):
            check_rounded(f"group_norm {IDS(dtype)} {N}x{S}x{C}/{G} silu={int(silu)} {'1L' if one else '2L'}",
                          run_group_norm(c, dtype, N, G, silu, one), c, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind,mod_rows", GN_MOD_CASES)
def test_group_norm_modulated_rounds_once(dtype, kind, mod_rows):
    N, S, C, G = GN_ONE_LAUNCH_SHAPES[0]
    assert gn_one_launch_ok(dtype, N, S, C, G)
    c = gn_case(dtype, N, S, C, G, True, kind, mod_rows)
    for one in (True, False):
        check_rounded(f"group_norm {IDS(dtype)} {kind} silu=1 {'1L' if one else '2L'}", run_group_norm(c, dtype, N, G, True, one), c, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_channel_norm_rounds_once(dtype):
    o = ops()
    c = cn_case(dtype)
    got = o.channel_norm(dev(c.x, dtype), c.gamma.to(DEV), c.beta.to(DEV), 1e-5, gelu=False).float().cpu()
    check_rounded(f"channel_norm {IDS(dtype)} {CN_SHAPE[0]}x{CN_SHAPE[1]}", got, c, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,N,scale", SOFTMAX_SHAPES)
def test_softmax_rows_rounds_once(dtype, M, N, scale):
    o = ops()
    c = softmax_case(dtype, M, N, scale)
    ld = (N + 7) // 8 * 8                                        # the kernel wants leading dimensions in whole 16-byte vectors: views of padded rows
    xb, yb = torch.full((M, ld), float("nan"), device=DEV, dtype=dtype), torch.zeros(M, ld, device=DEV, dtype=dtype)
    xb[:, :N] = dev(c.x, dtype)
    got = o.softmax_rows(xb[:, :N], c.scale, out=yb[:, :N]).float().cpu()
    check_rounded(f"softmax_rows {IDS(dtype)} {M}x{N}", got, c, dtype)


# =================================================================================================== family C: attention
# (B, heads, Lq, Lk0, Lk1, d).  "resident": a short context that attention_plan sends to the walk over several query tiles per block
# (the two-query-tiles-per-WAVE instantiation is not compiled in: attention.hip launch_attention2 pins QT = 1).
# measured rms ratio / rigorous budget fraction:
#   attention           bf16 rms 0.83 to 0.94, budget <= 0.61; f16 rms 0.81 to 0.95, budget <= 0.58; f32 rms 0.96 to 1.04, budget <= 0.11
#   temporal_attention  MFMA kernel: bf16 rms 1.00, budget <= 0.75; f16 rms 1.00, budget <= 0.83
#                       LDS kernel:  bf16 rms 1.00, budget 0.74; f16 rms 1.00, budget 0.66; f32 rms 0.99 to 1.01, budget <= 0.066
# f32 is measured against attn_model_f32, the kernels' own order of f32 sums; against torch's blocked matmul + expf the same outputs
# gave 1.15 (attention) and 1.61 (temporal, d = 256: 256 terms summed in order).
# (the flash form of attention.hip sits BELOW its model, as the same form does on the CPU; temporal.hip IS its model)
ATTN_CASES = {
    "single_150_d40": (2, 3, 150, 150, 0, 40),
    "single_77_d160": (1, 2, 77, 77, 0, 160),
    "single_12_d40": (8, 4, 12, 12, 0, 40),
    "two_segments": (2, 3, 100, 100, 45, 40),
    "resident": (20, 8, 256, 77, 0, 40),
}
TEMPORAL_MFMA = [(12, 40), (12, 80), (20, 40), (20, 80)]                  # (F, d): the MFMA kernel in the two-byte types
TEMPORAL_GENERIC = (24, 256)                                              # the LDS kernel in every type (f32 always takes it)
TEMPORAL_B, TEMPORAL_HW, TEMPORAL_HEADS = 2, 5, 3


def attn_math(qh, kh, vh, scale, p_dtype=None):
    """softmax(q k^T * scale) v over (..., L, d) operands in their own precision; p_dtype: the probabilities rounded to it.
    Returns (out, P |v|)."""
    p = torch.softmax(torch.matmul(qh, kh.transpose(-1, -2)) * scale, -1)
    if p_dtype is not None and p_dtype != torch.float32:
        p = p.to(p_dtype).to(qh.dtype)
    return torch.matmul(p, vh), torch.matmul(p, vh.abs())


LOG2E = 1.4426950408889634


def fma32(a, b, c):
    """a * b + c rounded once to f32, as v_fma_f32 / an f32 MFMA step does (the product of two f32 is exact in f64; the f64 rounding of
    the sum in between is 2^29 times finer than the f32 one)"""
    return (a.double() * b.double() + c.double()).float()


def dot_in_order(qh, kh):
    """q k^T over (..., L, d) f32 operands with d summed IN ORDER, one f32 fma per term: the score loop of both attention kernels
    in f32 (temporal.hip phase A / dot16<float>; attention.hip mma16<float>: chained v_mfma_f32_32x32x2_f32)"""
    acc = torch.zeros(*qh.shape[:-1], kh.shape[-2])
    for i in range(qh.shape[-1]):
        acc = fma32(qh[..., :, None, i], kh[..., None, :, i], acc)
    return acc


def pv_in_order(p, vh):
    """P V with the keys summed in order, one f32 fma per key"""
    acc = torch.zeros(*p.shape[:-1], vh.shape[-1])
    for j in range(p.shape[-1]):
        acc = fma32(p[..., :, j, None], vh[..., None, j, :], acc)
    return acc


def sum_in_order(p):
    acc = torch.zeros(p.shape[:-1])
    for j in range(p.shape[-1]):
        acc = acc + p[..., j]
    return acc


def attn_model_f32(qh, kh, vh, scale, kind):
    """The f32 mode of the two kernels as their code states it - f32 rounds no P, so what the model must share with the kernel is the
    ORDER of the f32 sums and the FORM of the exponential; torch's blocked matmul and its expf are more accurate than either and
    make the ratio measure the order, not a mistake (measured against that model: attention 1.15, temporal at d = 256 1.61).
      attention: scores in order over d; p = exp2(s * c - m * c) with c = scale * log2(e) folded, the argument ONE fma
                 (attention.hip:261, 475-485: v_pk_fma_f32 + v_exp_f32); P V and the row sum in order over the keys; O * (1 / l)
                 (attention.hip:618-627)
      temporal:  scores in order over d, times scale (temporal.hip:80-96); e = __expf(s - max) = exp2((s - max) * log2(e))
                 (temporal.hip:108); sum in order, w = e * (1 / sum) (109-111); P V in order over the frames (134-143)"""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    s = dot_in_order(qh, kh)
    if kind == "attention":
        c = f(scale) * f(LOG2E)
        m_sc = s.amax(-1, keepdim=True) * c
        e = torch.exp2(fma32(s, c, -m_sc))
        return pv_in_order(e, vh) * (1.0 / sum_in_order(e))[..., None]
    s = s * f(scale)
    e = torch.exp2((s - s.amax(-1, keepdim=True)) * f(LOG2E))
    return pv_in_order(e * (1.0 / sum_in_order(e))[..., None], vh)


def attn_finish(qh, kh, vh, scale, dtype, kind):
    r, pabsv = attn_math(qh.double(), kh.double(), vh.double(), scale)
    if dtype == torch.float32:
        return r, pabsv, attn_model_f32(qh, kh, vh, scale, kind)
    return r, pabsv, attn_math(qh, kh, vh, scale, dtype)[0].to(dtype)


@functools.lru_cache(maxsize=None)
def attn_case(dtype, name):
    B, heads, Lq, Lk0, Lk1, d = ATTN_CASES[name]
    g = gen(8009 + Lq + d)
    C_ = heads * d
    qq, k0, v0 = (q(torch.randn(B, L, C_, generator=g), dtype) for L in (Lq, Lk0, Lk0))
    k1 = v1 = None
    kk, vv = k0, v0
    if Lk1:
        k1, v1 = q(torch.randn(B, Lk1, C_, generator=g), dtype), q(torch.randn(B, Lk1, C_, generator=g), dtype)
        kk, vv = torch.cat([k0, k1], 1), torch.cat([v0, v1], 1)
    sp = lambda t: t.reshape(B, -1, heads, d).permute(0, 2, 1, 3)
    scale = f32c(d ** -0.5)
    r, pabsv, model = attn_finish(sp(qq), sp(kk), sp(vv), scale, dtype, "attention")
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B * Lq, C_)
    return NS(q=qq, k0=k0, v0=v0, k1=k1, v1=v1, scale=scale, r=back(r), pabsv=back(pabsv), model=back(model), L=Lk0 + Lk1, d=d,
              vmax=float(vv.abs().max()))


def vt_padded(v, dtype):
    """(B, L, C) -> V^T (B, C, ld) on the device, ld = L rounded up to 8, the pad columns NaN"""
    B, L, C_ = v.shape
    vt = torch.full((B, C_, (L + 7) // 8 * 8), float("nan"))
    vt[:, :, :L] = v.permute(0, 2, 1)
    return dev(vt, dtype)


def check_attention(label, got, c, dtype):
    frac = P.budget_fraction(got, c.r, P.attention_budget(c.r, c.pabsv, c.L, c.d, c.vmax, dtype))
    ratio = P.rms_ratio(got, c.model, c.r)
    report(label, budget=frac, rms=ratio)
    assert frac <= 1.0, f"{label}: {frac:.3f} of the rigorous budget"
    # against the model of the contract: two-byte types the NORMALISED P rounded to the dtype and everything else in f32 (the flash
    # form of attention.hip is held to it: tests/test_precision_ref_host.py), f32 the kernel's own order of sums (attn_model_f32)
    assert ratio <= RMS_CAP_C, f"{label}: rms error {ratio:.3f} x the contract model's (cap {RMS_CAP_C})"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(ATTN_CASES))
def test_attention_meets_its_rounding_contract(dtype, name):
    o = ops()
    B, heads, Lq, Lk0, Lk1, d = ATTN_CASES[name]
    pl = o.attention_plan(dtype=dtype, B=B, Lq=Lq, Lk0=Lk0, heads=heads, d=d, Lk1=Lk1)
    assert (pl[3] > 1) == (name == "resident"), pl
    c = attn_case(dtype, name)
    C_ = heads * d
    kw = {}
    if Lk1:
        kw = dict(k1=dev(c.k1.reshape(-1, C_), dtype), v1t=vt_padded(c.v1, dtype), Lk1=Lk1, seg1_div=1, seg1_first_batch=0)
    got = o.attention(dev(c.q.reshape(-1, C_), dtype), dev(c.k0.reshape(-1, C_), dtype), vt_padded(c.v0, dtype), Lk0, B=B, Lq=Lq, heads=heads,
                      d=d, scale=c.scale, **kw).float().cpu()
    check_attention(f"attention {IDS(dtype)} {name}", got, c, dtype)


@functools.lru_cache(maxsize=None)
def temporal_case(dtype, Fr, d):
    B, HW, heads = TEMPORAL_B, TEMPORAL_HW, TEMPORAL_HEADS
    C_ = heads * d
    qkv = q(torch.randn(B * Fr * HW, 3 * C_, generator=gen(8011 + Fr + d)), dtype)
    t = qkv.reshape(B, Fr, HW, 3, heads, d).permute(3, 0, 2, 4, 1, 5)      # (3, B, HW, heads, F, d)
    scale = f32c(d ** -0.5)
    r, pabsv, model = attn_finish(t[0], t[1], t[2], scale, dtype, "temporal")
    back = lambda u: u.permute(0, 3, 1, 2, 4).reshape(B * Fr * HW, C_)
    return NS(qkv=qkv, scale=scale, r=back(r), pabsv=back(pabsv), model=back(model), L=Fr, d=d, vmax=float(t[2].abs().max()))


def temporal_takes_mfma(dtype, Fr, d):
    """the dispatch of emo_temporal_attention (temporal.hip:329), mirrored: the MFMA kernel serves the two-byte types while its four
    wave-private V images - 16 or 32 frames x d two-byte channels + 64 bytes each - fit 64 KB; the LDS kernel serves the rest"""
    return dtype != torch.float32 and d % 8 == 0 and d <= 256 and 4 * (16 * (1 if Fr <= 16 else 2) * d * 2 + 64) <= 64 * 1024


def run_temporal(dtype, Fr, d, label):
    o = ops()
    assert temporal_takes_mfma(dtype, Fr, d) == (label == "mfma"), (dtype, Fr, d, label)
    c = temporal_case(dtype, Fr, d)
    got = o.temporal_attention(dev(c.qkv, dtype), TEMPORAL_B, Fr, TEMPORAL_HW, TEMPORAL_HEADS, d, c.scale).float().cpu()
    check_attention(f"temporal_attention {IDS(dtype)} {label} F={Fr} d={d}", got, c, dtype)


@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
@pytest.mark.parametrize("Fr,d", TEMPORAL_MFMA)
def test_temporal_attention_mfma_meets_its_rounding_contract(dtype, Fr, d):
    run_temporal(dtype, Fr, d, "mfma")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_temporal_attention_generic_meets_its_rounding_contract(dtype):
    run_temporal(dtype, *TEMPORAL_GENERIC, "generic")


@pytest.mark.parametrize("Fr,d", TEMPORAL_MFMA[:1] + TEMPORAL_MFMA[-1:])
def test_temporal_attention_f32_meets_its_rounding_contract(Fr, d):
    run_temporal(torch.float32, Fr, d, "generic")


# =================================================================================================== family D: every 16-bit input
# The f32-side allowance c(x) is the claim of common.h: rcp and exp2 at about one ulp each (silu, quick_gelu: 4 * 2^-24 |r|), the
# erf approximation of the two-byte GELU (|x| 1.5e-7 on top), tanh 4 * 2^-24 absolute, relu exact.
# measured share over the finite inputs (the budget fraction is 0.995 to 0.9994 everywhere: the half ulp of saturated outputs):
#   silu 3.2e-4 bf16 / 3.2e-5 f16 (ops.silu and ops.act alike); relu exact; tanh 0 / 0; gelu 1.8e-3 / 7.2e-3; quick_gelu 3.1e-4 / 3.2e-5
# GEGLU: f32-side error per unit value 1.84e-4 (bf16) / 1.86e-4 (f16) against the claimed 1.9e-4, on every tile; at gates up to 1/16 the
# output is within 0.73 ulp (the comment's "six ulps at 0.05" does not happen); the largest ulp count is 2009 f16 / 261 bf16 ulps at
# gate -3.94, where gelu is -1.6e-4 and the ABSOLUTE claim is larger than the value.
ACT_KINDS = ["silu", "relu", "tanh", "gelu", "quick_gelu"]
GEGLU_VALUES = [1.0, -1.0, 3.0]
GEGLU_CLAIM = 1.9e-4                                                      # common.h geglu_poly2: |gelu error| absolute
GEGLU_CHUNK = 8192


def all_patterns(dtype):
    """every 16-bit pattern of a two-byte type, as f32 values (CPU)"""
    return torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype).float()


def act_math(x, kind):
    """the activation in f64 with the limits at the infinities (x / (1 + exp(-x)) is NaN at -inf in floating point)"""
    x = x.double()
    if kind == "silu":
        r = x / (1 + torch.exp(-x))
    elif kind == "relu":
        r = torch.clamp(x, min=0.0)
        r = torch.where(torch.isnan(x), x, r)
    elif kind == "tanh":
        r = torch.tanh(x)
    elif kind == "gelu":
        r = 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))
    else:
        r = x / (1 + torch.exp(-1.702 * x))
    if kind in ("silu", "gelu", "quick_gelu"):
        r = torch.where(x == -float("inf"), torch.zeros_like(r), r)
    return r


F32_TINY = 2.0 ** -126                                                    # smallest normal f32


SIGMOID_FLUSH = {"silu": -87.0, "quick_gelu": -87.0 / 1.702}              # below these inputs exp(-x) passes 2^126


def act_allowance(x, r, kind):
    """c(x): the f32-side claim.  silu / quick_gelu: relative - and, ONLY below SIGMOID_FLUSH, |x| 2^-126: there 1 + exp(-x) is past
    2^126, its reciprocal is a subnormal f32, and `silu_f` (v_rcp_f32) and the division flush it to zero; only a bf16
    output (about 1e-37) can tell"""
    x, a = x.double(), r.abs()
    if kind in ("silu", "quick_gelu"):
        return 4 * P.U32 * a + torch.where(x < SIGMOID_FLUSH[kind], x.abs() * F32_TINY, torch.zeros_like(a))
    x = x.abs()
    if kind == "gelu":
        return x * 1.5e-7 + 4 * P.U32 * a
    return torch.full_like(a, 4 * P.U32 if kind == "tanh" else 0.0)


@functools.lru_cache(maxsize=None)
def act_case(dtype, kind):
    x = all_patterns(dtype)
    r = act_math(x, kind)
    model = {"silu": lambda t: t / (1 + torch.exp(-t)), "relu": torch.relu, "tanh": torch.tanh,           # the forms of common.h, in f32
             "gelu": lambda t: 0.5 * t * torch.erfc(-t * 0.70710678118654752440), "quick_gelu": lambda t: t / (1 + torch.exp(-1.702 * t))}[kind](x)
    return NS(x=x, r=r, model=model.to(dtype), finite=torch.isfinite(x))


def check_unary(label, got, c, dtype, kind):
    fin = c.finite
    r, g = c.r[fin], got.double()[fin]
    budget = 0.5 * P.ulp(r, dtype) * (1 + 2.0 ** -10) + act_allowance(c.x[fin], r, kind)
    err = (g - r).abs()
    frac = float((err / budget.clamp_min(1e-300)).max()) if kind != "relu" else float((err != 0).any())
    share = P.misrounded_share(g, r, dtype)
    report(label, budget=frac, share=share)
    assert bool(torch.isnan(got[torch.isnan(c.x)]).all()), f"{label}: NaN inputs must give NaN"
    assert not bool(torch.isnan(g).any()), f"{label}: NaN from a finite input"
    if kind == "relu":
        assert torch.equal(g, P.correctly_rounded(r, dtype).double()), f"{label}: relu is exact"
    assert bool((err <= budget).all()), f"{label}: {frac:.3f} of the budget at x = {float(c.x[fin][(err / budget.clamp_min(1e-300)).argmax()])}"
    assert share <= SHARE_CAP, f"{label}: misrounded share {share:.4f}"


@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
@pytest.mark.parametrize("kind", ACT_KINDS)
def test_act_over_every_16_bit_input(dtype, kind):
    o = ops()
    c = act_case(dtype, kind)
    check_unary(f"act {kind} {IDS(dtype)}", o.act(dev(c.x, dtype), kind).float().cpu(), c, dtype, kind)


@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
def test_silu_over_every_16_bit_input(dtype):
    o = ops()
    c = act_case(dtype, "silu")
    check_unary(f"silu {IDS(dtype)}", o.silu(dev(c.x, dtype)).float().cpu(), c, dtype, "silu")


@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
@pytest.mark.parametrize("kind", ACT_KINDS)
def test_act_at_the_infinities(dtype, kind):
    """+-inf map to the f64 limit of the activation: 0 / +inf (silu, relu, gelu, quick_gelu), +-1 (tanh)"""
    o = ops()
    x = torch.tensor([float("inf"), -float("inf")])
    want = act_math(x, kind)
    got = o.act(dev(x, dtype), kind).float().cpu().double()
    report(f"act {kind} {IDS(dtype)} at +inf, -inf", pos=float(got[0]), neg=float(got[1]))
    assert torch.equal(got, want), (kind, got.tolist(), want.tolist())
    if kind == "silu":
        assert torch.equal(o.silu(dev(x, dtype)).float().cpu().double(), want)


@functools.lru_cache(maxsize=None)
def geglu_case(dtype):
    """the identity-weight GEMM of tests/test_gpu_kernels.py test_geglu_gate_range_and_tails with EVERY 16-bit pattern as a gate:
    column 0 of A the gate, column 1 the value (1, -1, 3 in turn), W picks them into the 32 value / 32 gate rows"""
    gates = all_patterns(dtype)
    M, K = gates.numel(), 64
    vals = torch.tensor(GEGLU_VALUES)[torch.arange(M) % 3]
    a = torch.zeros(M, K)
    a[:, 0], a[:, 1] = gates, vals
    w = torch.zeros(64, K)
    w[:32, 1], w[32:, 0] = 1.0, 1.0
    g, v = gates.double(), vals.double()
    return NS(a=a, w=w, g=g, v=v, r=v * act_math(gates, "gelu"))


def run_geglu(c, dtype, tile=0):
    o = ops()
    wd = dev(c.w, dtype)
    outs = []
    for m0 in range(0, c.a.shape[0], GEGLU_CHUNK):
        got = o.gemm(dev(c.a[m0:m0 + GEGLU_CHUNK], dtype), wd, None, geglu=True, tile=tile).float().cpu()
        assert torch.equal(got.isnan(), got[:, :1].isnan().expand_as(got)) and torch.equal(got.nan_to_num(7.0), got[:, :1].nan_to_num(7.0).expand_as(got))
        outs.append(got[:, 0])
    return torch.cat(outs).double()


F32_HUGE = 2.0 ** 127      # |value * gate| from here on is not safe in f32: the product overflows


def geglu_run_and_split(dtype, tile):
    c = geglu_case(dtype)
    got = run_geglu(c, dtype, tile)
    fin = torch.isfinite(c.g)
    safe = fin & ((c.v * c.g).abs() < F32_HUGE)
    return c, got, P.correctly_rounded(c.r, dtype).double(), fin, safe


@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
@pytest.mark.parametrize("tile", [0, 2, 4])
def test_geglu_over_every_16_bit_gate(dtype, tile):
    """|got - v gelu(g)| <= half an ulp + |v| 1.9e-4 (1 + 2^-6) over every finite gate whose product with the value f32 can hold (all of
    them in f16); where v gelu(g) rounds to +-inf exactly that; beyond |g| = 9 exactly v g or 0; NaN gates give NaN.  Printed: the
    largest f32-side error per unit value (the claim is 1.9e-4) and the largest error in ulps of the OUTPUT - at gates up to 1/16,
    where about six f16 ulps are what the claim allows, and anywhere (the claim is absolute: the negative tail of gelu is smaller than it)."""
    c, got, want, fin, safe = geglu_run_and_split(dtype, tile)
    ok = safe & torch.isfinite(want)
    err = (got - c.r).abs()
    half = 0.5 * P.ulp(c.r, dtype)
    budget = half + c.v.abs() * GEGLU_CLAIM * (1 + 2.0 ** -6)
    nan_out = int(torch.isnan(got[safe]).sum())
    e, bdg = err[ok].nan_to_num(float("inf")), budget[ok]
    ulps = e / P.ulp(c.r[ok], dtype)
    small = ok & (c.g.abs() <= 2.0 ** -4) & (c.g.abs() >= 2.0 ** -10)
    report(f"geglu {IDS(dtype)} tile={tile}", budget=float((e / bdg).max()), f32_side_per_v=float(((e - half[ok]).clamp_min(0) / c.v[ok].abs()).max()),
           ulps_small_gates=float((err[small] / P.ulp(c.r[small], dtype)).max()), ulps_anywhere=float(ulps.max()), at_gate=float(c.g[ok][ulps.argmax()]),
           nan_from_finite=nan_out)
    assert bool(torch.isnan(got[torch.isnan(c.g)]).all())
    assert nan_out == 0, f"{nan_out} NaN outputs from finite gates, first at gate {float(c.g[safe][torch.isnan(got[safe])][0])}"
    assert torch.equal(got[safe & ~ok], want[safe & ~ok])                      # overflow of the two-byte type: the same infinity
    assert bool((e <= bdg).all()), f"geglu {IDS(dtype)}: {float((e / bdg).max()):.3f} of the budget"
    far = ok & (c.g.abs() > 9)
    assert torch.equal(got[far], want[far])                                  # the tails are exact: value * gate and 0
    assert torch.equal(got[c.g == 0], torch.zeros(int((c.g == 0).sum()), dtype=torch.float64))


# OPEN FINDING (bf16 only; f16 has no such gate): geglu_poly2 multiplies (value * gate) first, then by the clamped 0.5 + E: where
# |value * gate| >= 2^128 the product is +-inf in f32 and a NEGATIVE gate gives -inf * 0 = NaN where v gelu(g) is 0.  Measured: 71 of
# the 65536 gates (value 3, gate <= -1.15e38).  The order (v * x) * s keeps the dependent chain of the VALU-bound epilogue short;
# v * (x * s) would be exact there at the SAME instruction count, one more dependent multiply - the first thing to time and take.
@pytest.mark.parametrize("dtype", [pytest.param(torch.bfloat16, id="bf16", marks=pytest.mark.xfail(
    strict=True, reason="geglu_poly2: (value * gate) overflows f32 before the zero factor of the negative tail: 71 NaN outputs, gates <= -1.15e38 x value 3"))])
def test_geglu_gates_whose_product_with_the_value_overflows_f32(dtype):
    c, got, want, fin, safe = geglu_run_and_split(dtype, 0)
    rest = fin & ~safe
    assert int(rest.sum()) > 0
    nan_out = int(torch.isnan(got[rest]).sum())
    report(f"geglu {IDS(dtype)} |v g| >= 2^127", gates=int(rest.sum()), nan_from_finite=nan_out)
    assert torch.equal(got[rest], want[rest])                                  # +-inf where v g overflows the type, 0 in the negative tail


def test_convert_fp16_round_at_every_half_boundary():
    """emo_convert(fp16_round) f32 -> f32 through IEEE half: for every finite f16 pattern the value itself, the midpoint to its
    neighbour (a tie) and the f32 values either side of the midpoint must round as torch's f32 -> f16 cast does (one step, nearest
    even), bit for bit - the existing bit-for-bit test covers special values and random ones, not every boundary."""
    o = ops()
    pat = all_patterns(torch.float16)
    vals = torch.unique(pat[torch.isfinite(pat)].double())                   # sorted; +-0 once
    edge = torch.cat([torch.tensor([-65536.0]), vals, torch.tensor([65536.0])])
    mid = ((edge[:-1] + edge[1:]) / 2).float()                               # exact: one more bit than f16; +-65520 round to inf
    inf = torch.tensor(float("inf"))
    src = torch.cat([pat[torch.isfinite(pat)], mid, torch.nextafter(mid, inf), torch.nextafter(mid, -inf)])
    got = o.convert(src.to(DEV), torch.float32, fp16_round=True).cpu()
    want = src.half().float()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
