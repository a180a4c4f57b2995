"""Precision measures for the kernel tests (tests/test_gpu_precision.py, tests/test_precision_ref_host.py): plain torch on the CPU,
f64 throughout.  A kernel output `got` is compared with the f64 value `r` of the same operation on the same (quantised) inputs:

  ulp(r, dtype)                 spacing of dtype at |r|, floored at the subnormal spacing
  correctly_rounded(r, dtype)   f64 -> dtype, round to nearest even, ONE step (torch's own f64 -> bf16 / f16 casts go through f32)
  misrounded_share(got, r)      fraction of outputs that are not the correctly rounded r
  accum_budget(r, sabs, terms)  half an ulp for the one output rounding + the forward bound of `terms` f32 operations
  staged_budget(...)            the same with one documented inner rounding (the LDS-staged GEMM epilogue)
  attention_budget(...)         the same for the attention contract: P rounded to the dtype, everything else f32
  rms_ratio(got, model, r)      rms(got - r) / rms(model - r)

bf16 keeps its subnormals, as torch's casts do."""
import torch

MANT = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}        # explicit mantissa bits
EMIN = {torch.float32: -126, torch.bfloat16: -126, torch.float16: -14}  # exponent of the smallest normal
EMAX = {torch.float32: 127, torch.bfloat16: 127, torch.float16: 15}
U32 = 2.0 ** -24                                                         # unit roundoff of f32


def _f64(t):
    return t.detach().to("cpu", torch.float64) if isinstance(t, torch.Tensor) else torch.tensor(t, dtype=torch.float64)


def ulp(r, dtype):
    """spacing of `dtype` at |r| (f64 tensor): 2^(floor(log2 |r|) - mant), with the exponent held inside [emin, emax] - below the
    smallest normal the spacing is the subnormal one, at and beyond the largest finite value that of the top binade"""
    a = _f64(r).abs()
    _, e = torch.frexp(a)                     # a = m * 2^e, m in [0.5, 1): floor(log2 a) = e - 1
    ex = torch.where((a == 0) | ~torch.isfinite(a), torch.full_like(e, EMIN[dtype]), e - 1)
    ex = torch.where(torch.isinf(a), torch.full_like(ex, EMAX[dtype]), ex).clamp(EMIN[dtype], EMAX[dtype])
    return torch.ldexp(torch.ones_like(a), ex - MANT[dtype])


def correctly_rounded(r, dtype):
    """f64 -> dtype in one round-to-nearest-even step: r / ulp is exact in f64 (a power-of-two scaling of a 53-bit value onto at
    most 2^25 steps), torch.round rounds halves to even, and the product back is representable; what rounds past the largest
    finite value is +-inf (IEEE overflow).  NaN stays NaN.  Returned as a tensor of `dtype`."""
    r = _f64(r)
    u = ulp(r, dtype)
    v = torch.round(r / u) * u
    v = torch.where(v.abs() > torch.finfo(dtype).max, torch.copysign(torch.full_like(v, float("inf")), r), v)
    v = torch.where(torch.isfinite(r), v, r)
    return v.to(torch.float32).to(dtype)      # exact twice: v is a value of dtype


def misrounded_share(got, r, dtype=None):
    """the fraction of elements of got that are not correctly_rounded(r): value comparison, so +0 == -0; where r rounds to +-inf
    (or is NaN) got must be that exactly (asserted here), and those positions stay out of the share"""
    dtype = dtype or got.dtype
    want = correctly_rounded(r, dtype).double()
    g = _f64(got).reshape(want.shape)
    special = ~torch.isfinite(want)
    if bool(special.any()):
        gs, ws = g[special], want[special]
        assert torch.equal(torch.isnan(gs), torch.isnan(ws)) and torch.equal(gs[~torch.isnan(gs)], ws[~torch.isnan(ws)]), \
            "an output whose exact value rounds to inf / is NaN must be exactly that"
    n = int((~special).sum())
    return float(((g != want) & ~special).sum()) / max(n, 1)


def accum_budget(r, sabs, terms, dtype):
    """|got - r| allowed to a kernel that accumulates `terms` f32 operations and rounds ONCE to dtype: half an ulp of the output
    (2^-10 of slack for the f32 value the rounding actually sees) + the standard forward bound gamma_n * sum|terms| of a sum taken
    in any order, n * u with u doubled so that an MFMA accumulate that truncates is covered as well.  sabs = the expression of r
    on absolute values."""
    r, sabs = _f64(r), _f64(sabs)
    return 0.5 * ulp(r, dtype) * (1 + 2.0 ** -10) + 2.0 * terms * U32 * sabs


def staged_budget(r, pre, pre_scale, sabs, terms, dtype):
    """accum_budget for an epilogue that rounds TWICE: the value `pre` is packed to dtype first (half an ulp of it, carried through
    the factor pre_scale it is multiplied by afterwards), then the output is rounded"""
    return accum_budget(r, sabs, terms, dtype) + 0.5 * ulp(pre, dtype) * (1 + 2.0 ** -10) * abs(float(pre_scale))


def attention_budget(r, pabsv, L, d, vmax, dtype):
    """|got - r| for softmax(q k^T) v with the probabilities rounded to dtype (relative 2^-(mant + 1) each, against sum p |v|),
    scores / softmax / P.V in f32 (L + d operations), one output rounding; f16 adds the absolute error of probabilities that land in
    its subnormal range (2^-25 each, L of them, times max |v|).  f32 rounds no P."""
    r, pabsv = _f64(r), _f64(pabsv)
    p_round = 0.0 if dtype == torch.float32 else 2.0 ** -(MANT[dtype] + 1) * 1.01
    b = 0.5 * ulp(r, dtype) * (1 + 2.0 ** -10) + (p_round + 2.0 * (L + d) * U32) * pabsv
    if dtype == torch.float16:
        b = b + L * 2.0 ** -25 * float(vmax)
    return b


def rms(t):
    return float(_f64(t).pow(2).mean().sqrt())


def rms_ratio(got, model, r):
    """rms(got - r) / rms(model - r): how much further from the truth than the stated model of the contract"""
    r = _f64(r)
    den = rms(_f64(model).reshape(r.shape) - r)
    num = rms(_f64(got).reshape(r.shape) - r)
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))


def budget_fraction(got, r, budget):
    """max over elements of |got - r| / budget (<= 1 passes)"""
    r = _f64(r)
    return float(((_f64(got).reshape(r.shape) - r).abs() / budget).max())


def truncate(x, dtype):
    """f32 / f64 -> dtype by dropping bits (round toward zero): a mutant's rounding, never a kernel's"""
    x = _f64(x)
    u = ulp(x, dtype)
    return (torch.trunc(x / u) * u).to(torch.float32)
