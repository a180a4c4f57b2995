"""GPU sweeps of the norm kernels (csrc/norm.hip) over their launch geometry: the wide arm and the column parts of the two-launch
GroupNorm, statistics and apply passes cut into different numbers of row chunks, empty chunks, every instantiation of the one-launch
kernel, the group extremes, the coefficient table and the Linear fold reading the partials of a column-split tensor, and every
lanes-per-row choice of the LayerNorm up to the second trip of its grid.

The cases are the tables of tests/norm_sweep_cases.py; tests/test_host_logic.py checks on the CPU (emo_groupnorm_plan,
emo_layernorm_plan) that each runs on the arm it names and that together they reach every arm.  The C entries are called directly:
ops.group_norm picks the kernel itself, and a sweep must not leave that to chance.

Exact groups (the grid probe, run-to-run identity) compare bits.  The parity groups compare with F.group_norm / F.layer_norm in f64 on
the quantised rows at the TOL table of tests/test_gpu_kernels.py, and print the largest error as a fraction of that tolerance before
they assert it (pytest -s shows the figures)."""
import math

import pytest
import torch
import torch.nn.functional as F

from emote_hack_amd.synth import seeded_randn
from tests import norm_sweep_cases as S
from tests.test_gpu_kernels import DEV, TOL, ops      # noqa: F401  (TOL: the only parity tolerances used here)

pytestmark = pytest.mark.gpu

SENTINEL = 3.0                          # fills the buffers around a strided view (exact in every dtype)
PAD = 16                                # columns on either side of a column view: whole 16-byte vectors in every dtype
U32 = 2.0 ** -24                        # unit roundoff of f32
UNIT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))       # the value the entries receive (float eps)

GN_PAIRS = [(c, dt) for c in S.GN for dt in S.CLASS_DTYPES[c["cls"]]]
GN_IDS = [f"{S.gn_id(c)}-{str(dt)[6:]}" for c, dt in GN_PAIRS]
LN_PAIRS = [(c, dt) for c in S.LN for dt in S.CLASS_DTYPES[c["cls"]]]
LN_IDS = [f"{S.ln_id(c)}-{str(dt)[6:]}" for c, dt in LN_PAIRS]


def gn_case(name, dtype):
    return next(c for c in S.GN if c["name"] == name and dtype in S.CLASS_DTYPES[c["cls"]])


def dti(dtype):
    return {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[dtype]


def stream():
    return torch.cuda.current_stream().cuda_stream


def lib():
    from emote_hack_amd import _lib
    return _lib.load()


def ptr(t):
    return None if t is None else t.data_ptr()


def within(family, label, got, ref64, dtype, scale=1.0):
    """the assert_close condition |got - ref| <= atol * scale + rtol * |ref| of TOL[dtype], as the largest error over its tolerance"""
    tol = TOL[dtype]
    g = got.double()
    assert g.shape == ref64.shape and bool(torch.isfinite(g).all()), (family, label, "not finite")
    f = float(((g - ref64).abs() / (tol["atol"] * scale + tol["rtol"] * ref64.abs())).max())
    print(f"norm-sweep {family} | {label} | {str(dtype)[6:]} | {f:.4f} of tolerance")
    assert f <= 1.0, (family, label, dtype, f)
    return f


def bounded(family, label, err, bound):
    """|err| <= bound elementwise (a worked-out bound, not a tolerance): prints the largest ratio, then asserts it"""
    assert bool(torch.isfinite(err).all())
    f = float((err.abs() / bound.clamp_min(1e-300)).max())
    print(f"norm-sweep {family} | {label} | {f:.4f} of bound")
    assert f <= 1.0, (family, label, f)


# ------------------------------------------------------------------------------------------------------------------ GroupNorm
class Gn:
    """the GroupNorm entries on one case in one dtype; operands are (rows, C) tensors or column views (ld = stride(0))"""

    def __init__(self, c, dtype):
        self.c, self.dtype, self.lib = c, dtype, lib()
        self.N, self.S, self.C, self.G = c["N"], c["S"], c["C"], c["G"]
        self.shape = (self.N, self.S, self.C, self.G)
        self.NC, self.Cp, self.RP, self.ns, self.na, self.wide = c["two"]
        self.one_ok = bool(c["one"][0])
        self.written = self.N * self.ns * self.G * 2          # floats of the partials [n][chunk][G][2]

    def workspace(self, fill=float("nan"), guard=64):
        n = self.lib.emo_groupnorm_workspace_bytes(*self.shape) // 4
        assert n >= self.written
        return torch.full((n + guard,), fill, device=DEV, dtype=torch.float32)

    def stats(self, x, part):
        assert self.lib.emo_groupnorm_stats(ptr(x), x.stride(0), ptr(part), *self.shape, dti(self.dtype), stream()) == 0

    def apply(self, x, part, g, b, y, silu, mod=None):
        if mod is None:
            rc = self.lib.emo_groupnorm_apply(ptr(x), x.stride(0), ptr(part), ptr(g), ptr(b), ptr(y), y.stride(0), *self.shape, EPS, int(silu),
                                              dti(self.dtype), stream())
        else:
            rc = self.lib.emo_groupnorm_apply_mod(ptr(x), x.stride(0), ptr(part), ptr(g), ptr(b), ptr(mod), mod.stride(0), ptr(y), y.stride(0),
                                                  *self.shape, EPS, int(silu), dti(self.dtype), stream())
        assert rc == 0

    def one(self, x, g, b, y, silu, mod=None):
        if mod is None:
            rc = self.lib.emo_groupnorm(ptr(x), x.stride(0), ptr(g), ptr(b), ptr(y), y.stride(0), *self.shape, EPS, int(silu), dti(self.dtype), stream())
        else:
            rc = self.lib.emo_groupnorm_mod(ptr(x), x.stride(0), ptr(g), ptr(b), ptr(mod), mod.stride(0), ptr(y), y.stride(0), *self.shape, EPS,
                                            int(silu), dti(self.dtype), stream())
        assert rc == 0

    def coeffs(self, part, g, b, mod=None):
        coef = torch.full((self.N, 2 * self.C), float("nan"), device=DEV, dtype=torch.float32)
        if mod is None:
            rc = self.lib.emo_groupnorm_coeffs(ptr(part), ptr(g), ptr(b), ptr(coef), *self.shape, EPS, dti(self.dtype), stream())
        else:
            rc = self.lib.emo_groupnorm_coeffs_mod(ptr(part), ptr(g), ptr(b), ptr(mod), mod.stride(0), ptr(coef), *self.shape, EPS, dti(self.dtype),
                                                   stream())
        assert rc == 0
        return coef


def affine(C, seed):
    g, b = 1 + 0.1 * seeded_randn((C,), seed), 0.1 * seeded_randn((C,), seed + 1)
    return g.to(DEV), b.to(DEV)


def modulation(N, C, seed):
    """f32 (N, 2C) rows (scale | shift) as a column view of a wider buffer (ldmod > 2C, 16-byte aligned)"""
    buf = torch.full((N, 2 * C + 8), SENTINEL, device=DEV, dtype=torch.float32)
    mod = buf[:, 4:4 + 2 * C]
    mod.copy_(0.2 * seeded_randn((N, 2 * C), seed).to(DEV))
    return mod


def random_rows(c, dtype, seed=5):
    """the rows of test_groupnorm_one_launch - seeded_randn scaled per channel, plus 0.5 - with an offset of its own per (instance,
    group) on top (steps of 0.25, neighbours differ): statistics read from another group's slot cannot pass.  Quantised, on the device."""
    N, Sr, C, G = c["N"], c["S"], c["C"], c["G"]
    x = seeded_randn((N * Sr, C), seed) * (1 + torch.arange(C) % 7 * 0.2) + 0.5
    off = ((torch.arange(N * G) * 5) % 13 - 6).float().reshape(N, 1, G, 1) * 0.25
    return (x.reshape(N, Sr, G, C // G) + off).reshape(N * Sr, C).to(DEV).to(dtype)


def integer_rows(c, dtype, seed=17):
    """small integers (-4 .. 4: exact in every dtype, and every f32 sum and sum of squares of a chunk is exact in any order)"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, (c["N"] * c["S"], c["C"]), generator=gen, dtype=torch.int8).to(DEV).to(dtype)


def gn_ref64(x, c, g, b, eps=EPS):
    N, Sr, C, G = c["N"], c["S"], c["C"], c["G"]
    return F.group_norm(x.double().reshape(N, Sr, C).permute(0, 2, 1), G, g.double(), b.double(), eps).permute(0, 2, 1).reshape(N * Sr, C)


def modulated64(ref64, c, mod):
    N, Sr, C = c["N"], c["S"], c["C"]
    m = mod.double()
    return (ref64.reshape(N, Sr, C) * (1 + m[:, None, :C]) + m[:, None, C:]).reshape(N * Sr, C)


def act64(t, silu):
    return F.silu(t) if silu else t


def exact_stats64(x, c):
    """(N, G) mean and 1 / sqrt(var + eps) in f64 by the kernels' statement (E[x^2] - mean^2, clamped at 0) from exact sums"""
    N, Sr, C, G = c["N"], c["S"], c["C"], c["G"]
    u = x.double().reshape(N, Sr, G, C // G)
    count = float(Sr * (C // G))
    mean = u.sum((1, 3)) / count
    var = ((u * u).sum((1, 3)) / count - mean * mean).clamp_min(0.0)
    return mean, 1.0 / torch.sqrt(var + EPS32)


def modulated_affine32(g, b, mod, C):
    """gn_modulate's three f32 roundings: m = 1 + s, gamma' = gamma m, beta' = fma(beta, m, t) - per (instance, channel)"""
    m = 1.0 + mod[:, :C]
    return g[None] * m, (b[None].double() * m.double() + mod[:, C:].double()).float()


@pytest.mark.parametrize("c,dtype", GN_PAIRS, ids=GN_IDS)
def test_groupnorm_grid_probe(c, dtype):
    """a. emo_groupnorm_stats on integer rows into a NaN-filled workspace: every slot of the [n][chunk][G][2] partials the plan names
    holds EXACTLY the integer sum and sum of squares of its rows and group (an empty chunk its zeros), and nothing behind them is
    written - a chunk that skips its store, a column part offset into the wrong groups or a row counted twice shows here.  On the same
    partials the emo_groupnorm_coeffs / emo_groupnorm_coeffs_mod tables against the f64 statement from the exact sums:
    |d scale| <= 4 * 2^-24 |scale| and |d shift| <= 4 * 2^-24 (|mean scale| + |beta|) - the roundings of (float)mean, (float)rstd,
    rstd * gamma and the fma, a bound and not a measurement (the modulated table: on gn_modulate's f32 (gamma', beta'), which the
    header promises bit for bit) - and the (s, s, b, b) interleave of channel pairs."""
    k = Gn(c, dtype)
    N, Sr, C, G, ns = k.N, k.S, k.C, k.G, k.ns
    x = integer_rows(c, dtype)
    part = k.workspace()
    k.stats(x, part)
    written = part[:k.written].reshape(N, ns, G, 2)
    assert not bool(torch.isnan(written).any()), "a slot the plan says is written still holds its NaN"
    assert bool(torch.isnan(part[k.written:]).all()), "a store behind the partials"
    rows, live = S.chunking(Sr, ns)
    u = torch.zeros(N, ns * rows, C, device=DEV, dtype=torch.float64)
    u[:, :Sr] = x.double().reshape(N, Sr, C)
    u = u.reshape(N, ns, rows, G, C // G)
    want = torch.stack([u.sum((2, 4)), (u * u).sum((2, 4))], -1)
    assert torch.equal(written.double(), want)
    assert not bool(written[:, live:].any())
    assert torch.equal(written.double().sum(1), torch.stack([x.double().reshape(N, Sr, G, -1).sum((1, 3)), (x.double() ** 2).reshape(N, Sr, G, -1).sum((1, 3))], -1))

    g, b = affine(C, 21)
    mod = modulation(N, C, 23)
    mean, rstd = exact_stats64(x, c)
    mean_c, rstd_c = mean.repeat_interleave(C // G, 1), rstd.repeat_interleave(C // G, 1)            # (N, C)
    for label, m in (("coeffs", None), ("coeffs_mod", mod)):
        coef = k.coeffs(part, g, b, m).reshape(N, C // 2, 2, 2)
        got_scale, got_shift = coef[:, :, 0, :].reshape(N, C).double(), coef[:, :, 1, :].reshape(N, C).double()
        gp, bp = (g[None].expand(N, C), b[None].expand(N, C)) if m is None else modulated_affine32(g, b, m, C)
        scale = rstd_c * gp.double()
        shift = bp.double() - mean_c * scale
        bounded("coeffs", f"{S.gn_id(c)} {label} scale", got_scale - scale, 4 * U32 * scale.abs())
        bounded("coeffs", f"{S.gn_id(c)} {label} shift", got_shift - shift, 4 * U32 * ((mean_c * scale).abs() + bp.double().abs()))


@pytest.mark.parametrize("c,dtype", GN_PAIRS, ids=GN_IDS)
def test_groupnorm_parity(c, dtype):
    """b. random rows through emo_groupnorm_stats + emo_groupnorm_apply / _apply_mod (on EVERY case, those the one-launch kernel would
    serve included) and through emo_groupnorm / emo_groupnorm_mod where the plan says ok, with and without SiLU, against F.group_norm
    in f64 on the quantised rows at TOL; where both paths run they also agree with each other at TOL.  The wide, column-split,
    split-mismatch and empty-chunk cases run again on column views of wider buffers (the columns beside the view stay untouched) and
    in place."""
    k = Gn(c, dtype)
    N, Sr, C = k.N, k.S, k.C
    x = random_rows(c, dtype)
    g, b = affine(C, 6)
    mod = modulation(N, C, 9)
    base = gn_ref64(x, c, g, b)
    refs = {(False, False): base, (True, False): modulated64(base, c, mod)}
    name = S.gn_id(c)
    part = k.workspace()
    k.stats(x, part)
    for modded in (False, True):
        for silu in (False, True):
            ref = act64(refs[(modded, False)], silu)
            tag = f"{name}{' mod' if modded else ''}{' silu' if silu else ''}"
            two = torch.full_like(x, float("nan"))
            k.apply(x, part, g, b, two, silu, mod if modded else None)
            within("two-launch", tag, two, ref, dtype)
            if k.one_ok:
                one = torch.full_like(x, float("nan"))
                k.one(x, g, b, one, silu, mod if modded else None)
                within("one-launch", tag, one, ref, dtype)
                within("one-vs-two", tag, one, two.double(), dtype)
    if not S.gn_rerun_as_views(c):
        return
    xbuf = torch.full((N * Sr, C + 2 * PAD), SENTINEL, device=DEV, dtype=dtype)
    xv = xbuf[:, PAD:PAD + C]
    xv.copy_(x)
    part.fill_(float("nan"))
    k.stats(xv, part)
    for modded, silu in ((False, True), (True, False)):
        ref = act64(refs[(modded, False)], silu)
        tag = f"{name}{' mod' if modded else ''}{' silu' if silu else ''}"
        runs = [("two-launch", lambda a, y: k.apply(a, part, g, b, y, silu, mod if modded else None))]
        if k.one_ok:
            runs.append(("one-launch", lambda a, y: k.one(a, g, b, y, silu, mod if modded else None)))
        for family, run in runs:
            ybuf = torch.full((N * Sr, C + 3 * PAD), SENTINEL, device=DEV, dtype=dtype)           # ldy != ldx
            yv = ybuf[:, 2 * PAD:2 * PAD + C]
            run(xv, yv)
            within(family, tag + " views", yv, ref, dtype)
            assert bool((ybuf[:, :2 * PAD] == SENTINEL).all()) and bool((ybuf[:, 2 * PAD + C:] == SENTINEL).all())
            inplace = xbuf.clone()
            iv = inplace[:, PAD:PAD + C]
            run(iv, iv)
            within(family, tag + " in place", iv, ref, dtype)
            assert bool((inplace[:, :PAD] == SENTINEL).all()) and bool((inplace[:, PAD + C:] == SENTINEL).all())
    assert bool((xbuf[:, :PAD] == SENTINEL).all()) and bool((xbuf[:, PAD + C:] == SENTINEL).all()) and torch.equal(xv, x)


FOLD_COUTS = [(13, True), (5, False)]       # (Cout, bias): not a multiple of the 8 rows of a block; fewer than 8; a null bias
FOLD_GEMM_COUTS = [(12, True), (4, False)]  # the same through emo_gemm, whose per-instance weights need N % 4 == 0


@pytest.mark.parametrize("dtype", S.DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("cout,with_bias", FOLD_COUTS)
@pytest.mark.parametrize("name", ["fold_2560", "fold_2064"])
def test_groupnorm_fold_reads_split_partials(name, cout, with_bias, dtype):
    """c. emo_groupnorm_fold_linear on the partials of a column-split tensor (C = 2560, the fold's widest row: 2 parts in the 2-byte
    types, 4 in f32; C = 2064: a row that is no whole number of 64-lane trips), integer rows so that the statistics are exact, against
    the f64 statement directly:
      W'[n][o][c] = W gamma rstd rounded to the type: |d| <= (u_type + 3 * 2^-24) |W'| (the f32 roundings of rstd, gamma rstd and the
                    product, then the type's; + half the smallest f16 subnormal);
      b'[n][o]    = sum_c W beta - mean W' + bias over the W' the kernel stored: a lane adds K = ceil(C / (64 V)) V two-product terms
                    in f32, six shuffle levels and the bias follow, mean is rounded to f32:
                    |d| <= (K + 12) 2^-24 (sum |W beta| + sum |mean W'| + |bias|)."""
    c = gn_case(name, dtype)
    k = Gn(c, dtype)
    N, Sr, C, G = k.shape
    V = S.vec(c["cls"])
    assert k.NC > 1
    x = integer_rows(c, dtype)
    g, b = affine(C, 31)
    w = (seeded_randn((cout, C), 33) / C ** 0.5).to(DEV).to(dtype)
    bias = (0.1 * seeded_randn((cout,), 35)).to(DEV) if with_bias else None
    part = k.workspace()
    k.stats(x, part)
    wn = torch.full((N, cout, C), float("nan"), device=DEV, dtype=dtype)
    rb = torch.full((N, cout), float("nan"), device=DEV, dtype=torch.float32)
    assert k.lib.emo_groupnorm_fold_linear(ptr(part), ptr(g), ptr(b), ptr(w), ptr(bias), ptr(wn), ptr(rb), N, Sr, C, G, cout, EPS, dti(dtype),
                                           stream()) == 0
    mean, rstd = exact_stats64(x, c)
    mean_c, rstd_c = mean.repeat_interleave(C // G, 1), rstd.repeat_interleave(C // G, 1)            # (N, C)
    w64 = w.double()
    wp = w64[None] * (g.double() * rstd_c)[:, None, :]
    label = f"{S.gn_id(c)} Cout={cout}{'' if with_bias else ' no bias'} {str(dtype)[6:]}"
    bounded("fold", label + " weights", wn.double() - wp, (UNIT[dtype] + 3 * U32) * wp.abs() + 2.0 ** -25)
    terms = (w64 * b.double()).abs().sum(1)[None] + (mean_c[:, None, :] * wn.double()).abs().sum(2) + (bias.double().abs()[None] if with_bias else 0.0)
    rb64 = (w64 * b.double()).sum(1)[None] - (mean_c[:, None, :] * wn.double()).sum(2) + (bias.double()[None] if with_bias else 0.0)
    K = -(-C // (64 * V)) * V
    bounded("fold", label + " row bias", rb.double() - rb64, (K + 12) * U32 * terms)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("cout,with_bias", FOLD_GEMM_COUTS)
@pytest.mark.parametrize("name", ["fold_2560_gemm", "fold_2064_gemm"])
def test_groupnorm_fold_through_the_gemm(name, cout, with_bias, dtype):
    """c. the same widths through ops.gemm(w_slab_rows=S) on random rows against group_norm (f64) -> linear at the fold test's
    tolerance (TOL, atol x 2).  S = 256: the smallest weight slab emo_gemm takes."""
    o = ops()
    c = gn_case(name, dtype)
    N, Sr, C, G = c["N"], c["S"], c["C"], c["G"]
    assert c["two"][0] > 1
    x = random_rows(c, dtype, seed=41)
    g, b = affine(C, 43)
    w = (seeded_randn((cout, C), 45) / C ** 0.5).to(DEV).to(dtype)
    bias = (0.1 * seeded_randn((cout,), 47)).to(DEV) if with_bias else None
    ref = F.linear(gn_ref64(x, c, g, b, 1e-6), w.double(), bias.double() if with_bias else None)
    wn, rb = o.group_norm_fold_linear(x, g, b, N, G, 1e-6, w, bias)
    got = o.gemm(x, wn, rb, w_slab_rows=Sr)
    within("fold-gemm", f"{S.gn_id(c)} Cout={cout}{'' if with_bias else ' no bias'}", got, ref, dtype, scale=2.0)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("name", ["idle", "nc2_wide", "nc4", "g128_c2", "s1", "count1"])
def test_groupnorm_degenerate_statistics(name, dtype):
    """d. a constant instance (x = 0.5, eps 1e-5: the variance is 0, or clamps there) through both paths is finite and equals beta
    within TOL.  One row of one channel per group (count = 1) on random rows is beta as well; there the kernels' y = x a + (beta - mean a)
    with a = gamma / sqrt(eps) cancels two terms of |x a| up to ~3000, so the condition is TOL plus the two f32 roundings of that
    size, 2 * 2^-24 |x gamma| / sqrt(eps) - a bound from the formulation, not from a run."""
    c = gn_case(name, dtype)
    k = Gn(c, dtype)
    N, Sr, C = k.N, k.S, k.C
    g, b = affine(C, 51)
    want = b.double()[None].expand(N * Sr, C)
    inputs = [("constant", torch.full((N * Sr, C), 0.5, device=DEV, dtype=dtype))]
    if name == "count1":
        inputs.append(("random", random_rows(c, dtype, seed=53)))
    for what, x in inputs:
        def equals_beta(path, y):
            if what == "constant":
                return within("degenerate", f"{S.gn_id(c)} {what} {path}", y, want, dtype)
            tol = TOL[dtype]
            bound = tol["atol"] + tol["rtol"] * want.abs() + 2 * U32 * (x.double() * g.double()[None]).abs() / math.sqrt(EPS32)
            bounded("degenerate", f"{S.gn_id(c)} {what} {path} {str(dtype)[6:]}", y.double() - want, bound)
        part = k.workspace()
        k.stats(x, part)
        two = torch.full_like(x, float("nan"))
        k.apply(x, part, g, b, two, False)
        equals_beta("two-launch", two)
        if k.one_ok:
            one = torch.full_like(x, float("nan"))
            k.one(x, g, b, one, False)
            equals_beta("one-launch", one)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=lambda d: str(d)[6:])
def test_groupnorm_runs_are_identical(dtype):
    """f. fixed-order reductions: a split-mismatch case (256 statistics chunks, 257 apply chunks) and a one-launch case give the same
    bits twice."""
    c = gn_case("split", dtype)
    k = Gn(c, dtype)
    x = random_rows(c, dtype, seed=61)
    g, b = affine(k.C, 63)
    outs, parts = [], []
    for _ in range(2):
        part = k.workspace()
        k.stats(x, part)
        y = torch.full_like(x, float("nan"))
        k.apply(x, part, g, b, y, True)
        outs.append(y)
        parts.append(part[:k.written])
    assert torch.equal(parts[0], parts[1]) and torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0].float()).all())
    c = gn_case("r16" if dtype == torch.float32 else "r8", dtype)
    k = Gn(c, dtype)
    x = random_rows(c, dtype, seed=65)
    g, b = affine(k.C, 67)
    outs = []
    for _ in range(2):
        y = torch.full_like(x, float("nan"))
        k.one(x, g, b, y, True)
        outs.append(y)
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0].float()).all())


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
LN_RPF, LN_FRAMES = 3, 5                # rows per frame of the temporal-PE add: divides no wavefront's rows (64 .. 1)


def ln_rows(M, C, dtype, seed):
    """random rows with an offset of their own per row (made on the device: the largest tables are 25 M elements)"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn((M, C), generator=gen, device=DEV, dtype=torch.float32) * 2 + 0.3
    return (x + ((torch.arange(M, device=DEV) % 11) - 5).float()[:, None] * 0.3).to(dtype)


@pytest.mark.parametrize("c,dtype", LN_PAIRS, ids=LN_IDS)
def test_layernorm_lanes_per_row(c, dtype):
    """e. emo_layernorm and emo_layernorm_stats at every lanes-per-row choice, one row, a partly filled last wavefront and a row count
    past 4096 blocks (y is filled with NaN first: the rows of the second trip must be written), against F.layer_norm in f64 at TOL and
    the statistics at rtol 1e-4 / atol 1e-5 (test_layernorm_common_offset's); with the temporal-PE add at 3 rows per frame, on
    column views of wider buffers and in place."""
    L = lib()
    M, C = c["M"], c["C"]
    x = ln_rows(M, C, dtype, 71)
    g, b = affine(C, 73)
    ref = F.layer_norm(x.double(), (C,), g.double(), b.double(), EPS)
    name = f"{S.ln_id(c)} lpr{c['plan'][0]}"

    def run(a, y, pe=None):
        assert L.emo_layernorm(ptr(a), a.stride(0), ptr(g), ptr(b), ptr(y), y.stride(0), M, C, EPS, ptr(pe), LN_RPF if pe is not None else 0,
                               LN_FRAMES if pe is not None else 0, dti(dtype), stream()) == 0

    y = torch.full_like(x, float("nan"))
    run(x, y)
    within("layernorm", name, y, ref, dtype)
    if c["plan"][3]:
        first_trip = S.LN_MAXGRID * 4 * c["plan"][1]
        assert first_trip < M and bool(torch.isfinite(y[first_trip:].float()).all())

    stats = torch.full((M, 2), float("nan"), device=DEV, dtype=torch.float32)
    assert L.emo_layernorm_stats(ptr(x), C, ptr(stats), M, C, EPS, dti(dtype), stream()) == 0
    x64 = x.double()
    want = torch.stack([x64.mean(1), (x64.var(1, unbiased=False) + EPS).rsqrt()], 1)
    err = (stats.double() - want).abs() / (1e-5 + 1e-4 * want.abs())
    assert bool(torch.isfinite(stats).all())
    print(f"norm-sweep layernorm-stats | {name} | {str(dtype)[6:]} | {float(err.max()):.4f} of tolerance")
    assert float(err.max()) <= 1.0

    pe = seeded_randn((LN_FRAMES + 2, C), 75).to(DEV)
    fr = (torch.arange(M, device=DEV) // LN_RPF) % LN_FRAMES
    ref_pe = ref.to(dtype).double() + pe[fr].double()        # the add follows the rounding of the norm's output to the type
    y = torch.full_like(x, float("nan"))
    run(x, y, pe)
    within("layernorm", name + " pe", y, ref_pe, dtype)

    xbuf = torch.full((M, C + 2 * PAD), SENTINEL, device=DEV, dtype=dtype)
    xv = xbuf[:, PAD:PAD + C]
    xv.copy_(x)
    ybuf = torch.full((M, C + 3 * PAD), SENTINEL, device=DEV, dtype=dtype)
    yv = ybuf[:, 2 * PAD:2 * PAD + C]
    run(xv, yv)
    within("layernorm", name + " views", yv, ref, dtype)
    assert bool((ybuf[:, :2 * PAD] == SENTINEL).all()) and bool((ybuf[:, 2 * PAD + C:] == SENTINEL).all())
    sv = torch.full((M, 2), float("nan"), device=DEV, dtype=torch.float32)
    assert L.emo_layernorm_stats(ptr(xv), xv.stride(0), ptr(sv), M, C, EPS, dti(dtype), stream()) == 0
    assert torch.equal(sv, stats)
    run(xv, xv)
    within("layernorm", name + " in place", xv, ref, dtype)
    assert bool((xbuf[:, :PAD] == SENTINEL).all()) and bool((xbuf[:, PAD + C:] == SENTINEL).all())
