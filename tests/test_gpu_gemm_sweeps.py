"""Sweeps of the dense tile GEMM (csrc/gemm_impl.h) over what the UNet's own shapes never reach: ragged K in the buffer loaders, widths
and leading dimensions that take the scalar / the vector row epilogue, strided operands, rows below one tile, V^T stores whose quads
straddle batches, split-K with uneven and empty slices, GEGLU with a row bias.  The case tables are tests/gemm_sweep_cases.py;
tests/test_host_logic.py checks on the CPU (emo_gemm_plan) that they reach every instantiation and store path.

Every case runs twice where the epilogue allows it:
  * the GRID PROBE, exact: A is one-hot (row m has a single 1 at column m % K), W / bias / row bias / residual are multiples of 1/16
    small enough that every sum - in any order, through any path, split or not - is exactly representable in all three dtypes.  The
    output must equal W[n, m % K] + bias + row bias + residual, scaled, BIT FOR BIT: one dropped or doubled term, one chunk read
    from the wrong place, shows - where a tolerance would hide a dropped 8-element chunk of K.
  * random operands against F.linear in f64 on inputs quantised to the compute dtype, at the project's TOL.
A lives in a wider buffer whose padding [K, lda) and guard rows are NaN, W is followed by a NaN guard block; the output is a column
slice of a larger buffer filled with a sentinel bit pattern, with extra rows (batches) behind it: every element outside the view
must keep its bits."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_sweep_cases as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {torch.float32: dict(rtol=1e-3, atol=1e-4), torch.bfloat16: dict(rtol=3e-2, atol=3e-2), torch.float16: dict(rtol=5e-3, atol=5e-3)}
IDS = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
SENTINEL = {2: 0x5A5B, 4: 0x5A5B5C5D}


def ops():
    from emote_hack_amd import ops as o
    return o


def q(t, dtype):
    return t.to(dtype).float()


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def sentinel(shape, dtype):
    t = torch.empty(shape, device=DEV, dtype=dtype)
    bits(t).fill_(SENTINEL[t.element_size()])
    return t


def untouched(buf, keep):
    """every element of buf under the boolean mask keep still holds the sentinel bits"""
    return bool((bits(buf)[keep] == SENTINEL[buf.element_size()]).all())


def nan_padded(t, ld, guard_rows=4):
    """t (rows, w) on the device as a view of a (rows + guard_rows, ld) buffer whose every other element is NaN"""
    buf = torch.full((t.shape[0] + guard_rows, ld), float("nan"), device=DEV, dtype=t.dtype)
    buf[:t.shape[0], :t.shape[1]] = t.to(DEV)
    return buf[:t.shape[0], :t.shape[1]]


def grid(shape, gen, lim):
    """multiples of 1/16 in [-lim, lim]"""
    return torch.randint(-16 * lim, 16 * lim + 1, shape, generator=gen).float() / 16.0


def ln_fold(wt, bias, gamma, beta, dtype):
    """what unet._pack does: (W * gamma rounded to the compute dtype, its row sums, bias + W . beta)"""
    wp = (wt * gamma[None, :]).to(dtype)
    bp = wt.to(dtype).float() @ beta + (bias if bias is not None else 0)
    return wp, wp.float().sum(1), bp


class Operands:
    """The operands of one (dtype, M, N, K, lda, mode) and the f64 product; cases that differ in tile / leading dimensions / epilogue
    pieces share them."""
    cache = {}

    @classmethod
    def get(cls, c, mode):
        key = (c["dtype"], c["M"], c["N"], c["K"], c["lda_pad"], c["ln"], mode)
        if key not in cls.cache:
            if len(cls.cache) > 8:
                cls.cache.clear()
            cls.cache[key] = cls(c, mode)
        return cls.cache[key]

    def __init__(self, c, mode):
        dtype, M, N, K = c["dtype"], c["M"], c["N"], c["K"]
        g = torch.Generator(device="cpu").manual_seed(1000 + 7 * N + K)
        self.probe = mode == "probe"
        if self.probe:
            a = torch.zeros(M, K)
            a[torch.arange(M), torch.arange(M) % K] = 1.0
            w = grid((N, K), g, 2)
        else:
            a = q(torch.randn(M, K, generator=g) * (1.3 if c["ln"] else 1.0) + (1.5 * torch.randn(M, 1, generator=g) if c["ln"] else 0), dtype)
            w = torch.randn(N, K, generator=g) / math.sqrt(K)
        self.bias = grid((N,), g, 1) if self.probe else 0.1 * torch.randn(N, generator=g)
        lda = K + c["lda_pad"]
        self.a = nan_padded(a.to(dtype), lda, guard_rows=4 + 128 // lda)     # (the guard holds a whole ring stage behind the last row)
        self.ln = None
        if c["ln"]:
            gamma, beta = 1 + 0.2 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
            wq = q(w, dtype)
            self.y0 = F.linear(F.layer_norm(a, (K,), gamma, beta).double(), wq.double())
            self.y0_bias = self.y0 + self.bias.double()
            wp, cs, bp = ln_fold(w, self.bias, gamma, beta, dtype)
            wp0, cs0, bp0 = ln_fold(w, None, gamma, beta, dtype)
            self.ln = dict(cs=cs.to(DEV).contiguous(), bias=bp.to(DEV).contiguous(), bias0=bp0.to(DEV).contiguous(),
                           stats=ops().layer_norm_stats(self.a, 1e-5))
            w_dev = wp
        else:
            w_dev = q(w, dtype).to(dtype)
            self.y0 = a.double() @ w_dev.double().t()
            self.y0_bias = self.y0 + self.bias.double()
        flat = torch.full((N * K + 4096,), float("nan"), device=DEV, dtype=dtype)      # W and a NaN guard block behind it
        flat[:N * K] = w_dev.reshape(-1).to(DEV)
        self.w = flat[:N * K].view(N, K)
        self.bias_d = self.bias.to(DEV)
        self.gen = g
        self.extra = {}

    def rowbias(self, rpb, M, N):
        if ("rb", rpb) not in self.extra:
            nb = (M + rpb - 1) // rpb
            self.extra[("rb", rpb)] = grid((nb, N), self.gen, 1) if self.probe else torch.randn(nb, N, generator=self.gen)
        return self.extra[("rb", rpb)]

    def residual(self, M, n_out, dtype):
        if ("res", n_out) not in self.extra:
            self.extra[("res", n_out)] = grid((M, n_out), self.gen, 2) if self.probe else q(torch.randn(M, n_out, generator=self.gen), dtype)
        return self.extra[("res", n_out)]


def run_case(case, mode, tol_scale=1.0, check_split1=False):
    """launch one case of tests/gemm_sweep_cases.py and check it; returns the output view (device)"""
    o = ops()
    c, g = S.full(case), S.geometry(case)
    dtype, M, N, K = c["dtype"], c["M"], c["N"], c["K"]
    n_out = g["n_out"]
    op = Operands.get(c, mode)
    kw = dict(tile=c["tile"], geglu=c["geglu"], out_scale=c["out_scale"])
    y = (op.y0_bias if c["bias"] else op.y0).clone()
    bias = op.bias_d if c["bias"] else None
    if c["ln"]:
        kw["ln"] = (op.ln["cs"], op.ln["stats"])
        bias = op.ln["bias"] if c["bias"] else op.ln["bias0"]
    if c["rowbias"]:
        rpb = c["rowbias"][0]
        rb = op.rowbias(rpb, M, N)
        y = y + rb.double()[torch.arange(M) // rpb]
        kw.update(rowbias=nan_padded(rb, g["ld_rowbias"], guard_rows=0), rows_per_batch=rpb)
    if c["geglu"]:
        y = y.reshape(M, N // 64, 2, 32)
        y = (y[:, :, 0] * F.gelu(y[:, :, 1])).reshape(M, n_out)
    res = None
    if c["residual"]:
        r = op.residual(M, n_out, dtype)
        y = y + r.double()
        if c["residual"] == 1:
            res = nan_padded(r.to(dtype), g["ldr"], guard_rows=0)
    y = y * c["out_scale"]
    split = c["split_k"]
    if split is None:
        split = S.plan(case)[4]
    nws = max(split, 1) * M * N
    launches = 2 if split > 1 else 1
    outs = []
    for rep in range(launches):
        if split > 1:
            kw["workspace"] = torch.full((nws,), float("nan"), device=DEV, dtype=torch.float32)   # an unwritten slab shows
        if c["trans"]:
            L, nb = c["trans"], M // c["trans"]
            buf = sentinel((nb + 1, N, g["t_ld"]), dtype)
            o.gemm(op.a, op.w, bias, out=buf, transpose_rows=L, transpose_ld=g["t_ld"], split_k=split, **kw)
            keep = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
            keep[:nb, :, :L] = False
            assert untouched(buf, keep), f"{case}: wrote outside the V^T view (pad columns / past the last batch)"
            got = buf[:nb, :, :L].permute(0, 2, 1).reshape(M, N)
        else:
            vt_cols = c["vt"][0] if c["vt"] else 0
            width = n_out - vt_cols
            buf = sentinel((M + 3, g["ldc"]), dtype)
            view = buf[:M, g["c0"]:g["c0"] + width]
            if c["residual"] == 2:
                view.copy_(op.residual(M, n_out, dtype).to(DEV).to(dtype))
                res = view
            keep = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
            keep[:M, g["c0"]:g["c0"] + width] = False
            if vt_cols:
                L, nb = c["vt"][1], M // c["vt"][1]
                vbuf = sentinel((nb + 1, vt_cols, g["t_ld"]), dtype)
                both = o.gemm(op.a, op.w, bias, out=view, vt_cols=vt_cols, vt_rows=L, vt_ld=g["t_ld"], vt_out=vbuf[:nb], **kw)
                assert both is not None, f"{case}: the split store is not served"
                vkeep = torch.ones(vbuf.shape, dtype=torch.bool, device=DEV)
                vkeep[:nb, :, :L] = False
                assert untouched(vbuf, vkeep), f"{case}: wrote outside the V^T view"
                got = torch.cat([view, vbuf[:nb, :, :L].permute(0, 2, 1).reshape(M, vt_cols)], 1)
            else:
                o.gemm(op.a, op.w, bias, out=view, residual=res, split_k=split, **kw)
                got = view
            assert untouched(buf, keep), f"{case}: wrote outside the M x n_out view"
        outs.append(got.float().cpu())
    got = outs[0]
    if launches == 2:
        assert torch.equal(bits(outs[0]), bits(outs[1])), f"{case}: split-K is not deterministic"
    if mode == "probe":
        want = y.to(dtype).float()
        bad = got != want
        assert not bool(bad.any()), (f"{case}: grid probe, {int(bad.sum())} of {bad.numel()} elements differ, first at "
                                     f"{bad.nonzero()[0].tolist()}: got {got[bad][0].item()} want {want[bad][0].item()}")
    else:
        tol = TOL[dtype]
        try:
            torch.testing.assert_close(got, y.float(), rtol=tol["rtol"], atol=tol["atol"] * tol_scale)
        except AssertionError as e:
            raise AssertionError(f"{case}: {e}") from None
    if check_split1 and split > 1 and not c["trans"]:
        one = sentinel((M, n_out), dtype)
        if c["residual"] == 2:
            one.copy_(op.residual(M, n_out, dtype).to(DEV).to(dtype))
        kw.pop("workspace", None)
        o.gemm(op.a, op.w, bias, out=one, residual=one if c["residual"] == 2 else res, split_k=1, **kw)
        tol = TOL[dtype]
        torch.testing.assert_close(got, one.float().cpu(), rtol=tol["rtol"], atol=tol["atol"] * tol_scale)
    return got


def sweep(cases, modes, tol_scale=1.0, **kw):
    for case in cases:
        for mode in modes:
            run_case(case, mode, tol_scale=tol_scale, **kw)


BOTH = ("probe", "random")
# (the grid probe is exact only where the epilogue is sums and one final rounding: not through GELU or the LayerNorm fold)
LN_SCALE = lambda dtype: 2.0 if dtype != torch.float32 else 1.0      # as tests/test_gpu_kernels.py test_gemm_layernorm_fold


# ---- a. K sweep ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_k_tails_column_probe_and_random(dtype):
    """K in {V, 2V, BK-V, BK, BK+V, 2BK-V, 2BK+V, 5BK+3V} on every tile hint, lda > K (NaN padding) and lda == K: C[m, n] must be
    W[n, m % K] bit for bit - every 16-byte chunk of every stage, the ragged last stage included, lands where it belongs and the
    chunks past K read zero, not the row's padding or the next row."""
    sweep(S.k_cases(dtype), BOTH)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_k_tails_with_the_layernorm_fold(dtype):
    sweep(S.k_ln_cases(dtype), ("random",), tol_scale=LN_SCALE(dtype))


# ---- b. N and leading dimensions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", list(S.N_EPILOGUES))
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_widths_and_leading_dimensions(dtype, epi):
    """N in 1 .. 321 x (ldc, ldr) in three alignment classes x tiles: the LDS-staged, the vector-row and the scalar-row epilogue, each
    with bias / row bias (uniform over a tile or not, ld_rowbias aligned or not) / residual / in-place residual / out_scale; out is
    a column slice of a sentinel-filled buffer."""
    sweep(S.n_cases(dtype, epi), BOTH)


@pytest.mark.parametrize("epi", list(S.N_GEGLU_EPILOGUES))
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_widths_geglu(dtype, epi):
    sweep(S.n_geglu_cases(dtype, epi), ("random",))


@pytest.mark.parametrize("epi", list(S.N_LN_EPILOGUES))
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_widths_layernorm_fold(dtype, epi):
    sweep(S.n_ln_cases(dtype, epi), ("random",), tol_scale=LN_SCALE(dtype))


# ---- c. M edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_row_counts_below_and_around_a_tile(dtype):
    """M in {1, 31, 32, 33, 63, 65, 127, 129, 255, 257} on every tile hint (the phase main loop included), bias + residual; nothing
    below row M is written."""
    sweep(S.m_cases(dtype), BOTH)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_row_counts_with_the_layernorm_fold(dtype):
    sweep(S.m_ln_cases(dtype), ("random",), tol_scale=LN_SCALE(dtype))


# ---- d. V^T stores ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("epi", list(S.T_EPILOGUES))
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_transposed_store_batch_lengths(dtype, epi, ln):
    """t_rows in {1, 3, 48, 50, 64, 77} over 7 batches (quads of 4 rows straddle batch boundaries unless t_rows % 4 == 0), t_ld a
    multiple of 4 or not, ragged N, bias / row bias / out_scale: the pad columns [t_rows, t_ld) and the batch behind the last keep
    their bits."""
    sweep(S.t_cases(dtype, epi, ln), ("random",) if ln else BOTH, tol_scale=LN_SCALE(dtype) if ln else 1.0)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_merged_qkv_with_a_narrow_v_block(dtype):
    sweep(S.vt_cases(dtype), ("random",), tol_scale=LN_SCALE(dtype))


# ---- e. split-K ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("large", [False, True], ids=["small_m", "many_tiles"])
@pytest.mark.parametrize("form", list(S.SPLIT_FORMS))
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_split_k_slices(dtype, form, large):
    """Even, uneven, trailing-empty and more-slices-than-stages splits of a ragged K, every form of the reduce kernel's epilogue,
    a NaN-filled workspace in front of every call (a slice that does not write its slab shows), two calls bit for bit, and the
    single-pass result at TOL."""
    assert any(S.split_empty(nk, s) for nk, s in S.SPLITS) and any(s > nk for nk, s in S.SPLITS)
    sweep(S.split_cases(dtype, form, large), ("random",) if form == "geglu" else BOTH, check_split1=True)


def test_split_k_planned_with_an_empty_slice():
    """The planner's own `s <= nk / 4` rule can pick a split whose last slice is empty; the shapes the CPU search finds
    (tests/gemm_sweep_cases.py planned_empty_slices) run at the planned setting."""
    hits = S.planned_empty_slices()
    assert hits, "the search found no planned split with an empty slice: update this test and say so"
    seen, picked = set(), []
    for h in hits:        # one per (dtype, long K or not)
        k = (h["dtype"], h["_nk"] >= 41)
        if k not in seen:
            seen.add(k)
            picked.append({a: b for a, b in h.items() if not a.startswith("_")})
    sweep(picked, BOTH, check_split1=True)


# ---- f. GEGLU with a row bias ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_geglu_row_bias_reaches_the_gate_columns(dtype):
    """emo_hip.h orders the epilogue + bias[N], + rowbias[..][N], GEGLU: the gate columns carry the row bias too - on every path (row
    bias in the accumulators, both branches of the row epilogue, the split-K reduce kernel)."""
    cases = S.geglu_rowbias_cases(dtype)
    pl = {S.plan(c)[5:8] for c in cases}
    assert {p[2] for p in pl} == {0, 1} and {p[0] for p in pl} >= {1, 2, 5}, pl
    sweep(cases, ("random",), check_split1=True)


# ---- g. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched():
    """emo_gemm returns the statuses emo_gemm_plan reports (tests/test_boundary.py) before any launch: the output keeps its bits."""
    import ctypes as C
    from emote_hack_amd import _lib
    lib, o = _lib.load(), ops()
    dtype = torch.bfloat16
    M, N, K = 64, 128, 128
    a = torch.ones(M, K + 8, device=DEV, dtype=dtype)
    w = torch.ones(N, K, device=DEV, dtype=dtype)
    ws = torch.zeros(4 * M * N, device=DEV, dtype=torch.float32)
    cs, st = torch.zeros(N, device=DEV), torch.zeros(M, 2, device=DEV)
    out = sentinel((M + 1, N + 8), dtype)

    def call(**kw):
        p = _lib.GemmParams()
        base = dict(A=a.data_ptr(), lda=K + 8, W=w.data_ptr(), C=out.data_ptr(), ldc=N + 8, M=M, N=N, K=K, out_scale=1.0, dtype=_lib.EMO_BF16)
        base.update(kw)
        for k, v in base.items():
            setattr(p, k, v)
        plan = (C.c_int * 8)(*([-7] * 8))
        rc_plan = lib.emo_gemm_plan(C.byref(p), plan)
        rc = lib.emo_gemm(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == rc_plan, (kw, rc, rc_plan)
        if rc != 0:
            assert list(plan) == [-7] * 8, kw
        return rc

    refused = [dict(K=K - 4), dict(lda=K + 4), dict(A=a.data_ptr() + 2), dict(W=w.data_ptr() + 8), dict(C=out.data_ptr() + 4),
               dict(geglu=1, N=96), dict(split_k=2, workspace=None), dict(split_k=2, workspace=ws.data_ptr(), N=126),
               dict(ln_colsum=cs.data_ptr(), ln_stats=st.data_ptr(), split_k=2, workspace=ws.data_ptr()),
               dict(ln_colsum=cs.data_ptr()), dict(ln_stats=st.data_ptr()),
               dict(w_slab_rows=128, w_slab_stride=N * K), dict(w_slab_rows=256, w_slab_stride=N * K, M=256 + 64),
               dict(vt=out.data_ptr(), vt_col0=64, t_rows=64, t_ld=64, t_batch_stride=64 * 64)]       # vt without the LayerNorm fold
    for kw in refused:
        assert call(**kw) < 0, kw
        assert untouched(out, torch.ones(out.shape, dtype=torch.bool, device=DEV)), kw
    assert call() == 0
    assert not untouched(out, torch.ones(out.shape, dtype=torch.bool, device=DEV))
