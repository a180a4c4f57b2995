"""Case tables of the dense-GEMM sweeps, shared by tests/test_gpu_gemm_sweeps.py (which launches them) and the CPU coverage test in
tests/test_host_logic.py (which asks emo_gemm_plan what each would launch).  Plain data, no device needed.

A case is a dict: dtype, M, N, K, tile (emo_gemm_params.tile hint) and the optional keys of DEFAULTS.  `geometry(case)` turns the
alignment CLASSES a case names into the leading dimensions both sides use; `plan_kwargs(case)` is the ops.gemm_plan call of a case.
V = elements per 16 bytes, BK = k-values per 128-byte ring stage."""
import torch

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TILE_BM = {1: 64, 2: 128, 3: 128, 4: 256, 5: 256, 6: 256, 7: 256}
ALL_HINTS = (0, 1, 2, 3, 4, 5, 6, 7)
LD_CLASSES = ("odd", "q4", "q8")       # leading dimension: not a multiple of 4 | a multiple of 4 but not of 8 | a multiple of 8

DEFAULTS = dict(lda_pad=0,             # lda = K + lda_pad (elements; a multiple of V)
                ld="q8",               # class of ldc and ldr (row-major) or of t_ld (V^T)
                bias=False,
                rowbias=None,          # (rows_per_batch, class of ld_rowbias: "q4" | "odd")
                residual=0,            # 0 none | 1 its own buffer | 2 aliases the output (in place)
                out_scale=1.0, geglu=False, ln=False,
                trans=0,               # t_rows of a V^T store (transpose_out)
                split_k=1,             # 1 single pass | S pinned | None = the planner's
                vt=None)               # (vt_cols, vt_rows): merged q | k | v, the last vt_cols columns stored transposed


def vec(dtype):
    return 4 if dtype == torch.float32 else 8


def bk(dtype):
    return 32 if dtype == torch.float32 else 64


def full(case):
    c = dict(DEFAULTS)
    c.update(case)
    return c


def ld_of(cls, width):
    """the smallest leading dimension >= width + 3 of an alignment class"""
    ld = width + 3
    ok = {"odd": lambda x: x % 4 != 0, "q4": lambda x: x % 8 == 4, "q8": lambda x: x % 8 == 0}[cls]
    while not ok(ld):
        ld += 1
    return ld


def geometry(case):
    """Leading dimensions of a case: lda, c0 (first output column inside the wider output buffer: C stays 16-byte aligned), ldc, ldr,
    ld_rowbias, t_ld, n_out."""
    c = full(case)
    V = vec(c["dtype"])
    n_out = c["N"] // 2 if c["geglu"] else c["N"]
    g = dict(lda=c["K"] + c["lda_pad"], n_out=n_out, c0=2 * V)
    width = n_out - (c["vt"][0] if c["vt"] else 0)
    g["ldc"] = ld_of(c["ld"], g["c0"] + width)
    g["ldr"] = g["ldc"] if c["residual"] == 2 else ld_of(c["ld"], n_out)
    if c["rowbias"]:
        g["ld_rowbias"] = ld_of(c["rowbias"][1], c["N"] - 3)      # >= N
    if c["trans"]:
        g["t_ld"] = ld_of(c["ld"], c["trans"] - 3)                 # >= t_rows
    if c["vt"]:
        g["t_ld"] = ld_of(c["ld"], c["vt"][1] - 3)
    return g


def plan_kwargs(case):
    c, g = full(case), geometry(case)
    kw = dict(dtype=c["dtype"], M=c["M"], N=c["N"], K=c["K"], lda=g["lda"], bias=c["bias"], geglu=c["geglu"], out_scale=c["out_scale"],
              ln=c["ln"], tile=c["tile"], split_k=c["split_k"])
    if c["rowbias"]:
        kw.update(rowbias=True, rows_per_batch=c["rowbias"][0], ld_rowbias=g["ld_rowbias"])
    if c["trans"]:
        kw.update(transpose_rows=c["trans"], transpose_ld=g["t_ld"])
    else:
        kw.update(ldc=g["ldc"])
    if c["residual"]:
        kw.update(residual=True, ldr=g["ldr"])
    if c["vt"]:
        kw.update(vt_cols=c["vt"][0], vt_rows=c["vt"][1], vt_ld=g["t_ld"])
    return kw


def plan(case):
    from emote_hack_amd import ops
    return ops.gemm_plan(**plan_kwargs(case))


# ---- a. K sweep -------------------------------------------------------------------------------------------------------------
def k_values(dtype):
    V, BK = vec(dtype), bk(dtype)
    return [V, 2 * V, BK - V, BK, BK + V, 2 * BK - V, 2 * BK + V, 5 * BK + 3 * V]


def k_rows(K):
    """M >= K (every column of A gets a one-hot row) and not a multiple of any tile height"""
    M = max(K, 64) + 37
    return M if M % 64 else M + 8


K_N = 72


def k_cases(dtype):
    V = vec(dtype)
    out = []
    for K in k_values(dtype):
        for tile in ALL_HINTS:
            for lda_pad in (3 * V, 0):
                out.append(dict(dtype=dtype, M=k_rows(K), N=K_N, K=K, tile=tile, lda_pad=lda_pad))
    return out


def k_ln_cases(dtype):
    V, BK = vec(dtype), bk(dtype)
    return [dict(dtype=dtype, M=k_rows(K), N=K_N, K=K, tile=tile, lda_pad=V, ln=True, bias=True)
            for K in (BK + V, 5 * BK + 3 * V) for tile in ALL_HINTS]


# ---- b. N and leading-dimension sweep, row-major -------------------------------------------------------------------------------
N_VALUES = (1, 2, 3, 4, 5, 12, 30, 33, 63, 65, 68, 100, 127, 129, 132, 161, 254, 321)
N_GEGLU = (64, 192, 320)               # GEGLU needs N % 64 == 0: n_out 32 / 96 / 160
N_M = 300                              # two batches of 256 rows (the last one ragged), three of 100
N_TILES = (1, 2, 3, 4, 5, 6)
# epilogue pieces: name -> case keys.  rows_per_batch 256 is a multiple of every tile height (the row bias then starts the
# accumulators where N and ld_rowbias allow), 100 of none
N_EPILOGUES = {
    "plain": dict(),
    "bias": dict(bias=True),
    "rb_tile": dict(bias=True, rowbias=(256, "q4")),
    "rb_tile_oddld": dict(rowbias=(256, "odd")),
    "rb_ragged": dict(rowbias=(100, "q4")),
    "rb_ragged_oddld": dict(bias=True, rowbias=(100, "odd")),
    "res": dict(residual=1, out_scale=0.5),
    "inplace": dict(bias=True, residual=2),
}
N_GEGLU_EPILOGUES = {"plain": dict(), "bias": dict(bias=True), "res": dict(bias=True, residual=1, out_scale=0.5)}
N_LN_EPILOGUES = {"bias": dict(bias=True), "rb_tile": dict(bias=True, rowbias=(256, "q4")), "rb_ragged": dict(rowbias=(100, "q4")),
                  "res": dict(bias=True, residual=1, out_scale=0.5)}


def n_K(dtype):
    return bk(dtype) + vec(dtype)      # one full stage + a ragged one


def n_cases(dtype, epi):
    out = []
    for N in N_VALUES:
        for ld in LD_CLASSES:
            for tile in N_TILES + ((0, 7) if epi == "plain" else ()):
                out.append(dict(dtype=dtype, M=N_M, N=N, K=n_K(dtype), tile=tile, ld=ld, **N_EPILOGUES[epi]))
    return out


def n_geglu_cases(dtype, epi):
    return [dict(dtype=dtype, M=N_M, N=N, K=n_K(dtype), tile=tile, ld=ld, geglu=True, **N_GEGLU_EPILOGUES[epi])
            for N in N_GEGLU for ld in LD_CLASSES for tile in (0, 2, 4, 7)]


def n_ln_cases(dtype, epi):
    return [dict(dtype=dtype, M=N_M, N=N, K=n_K(dtype), tile=tile, ld=ld, ln=True, **N_LN_EPILOGUES[epi])
            for N in N_VALUES if N % 4 == 0 for ld in LD_CLASSES for tile in N_TILES]


# ---- c. M edges ----------------------------------------------------------------------------------------------------------------
M_VALUES = (1, 31, 32, 33, 63, 65, 127, 129, 255, 257)
M_N = (200, 132, 131)                  # 2-byte types: n_out % 8 == 0 (LDS-staged), % 8 == 4 (vector row), odd (scalar row)


def m_cases(dtype):
    # K = two whole stages: hint 7 keeps the phase main loop
    return [dict(dtype=dtype, M=M, N=N, K=2 * bk(dtype), tile=tile, bias=True, residual=1)
            for M in M_VALUES for N in M_N for tile in ALL_HINTS]


def m_ln_cases(dtype):
    return [dict(dtype=dtype, M=M, N=M_N[0], K=2 * bk(dtype), tile=tile, bias=True, ln=True) for M in M_VALUES for tile in ALL_HINTS]


# ---- d. V^T stores ---------------------------------------------------------------------------------------------------------------
T_ROWS = (1, 3, 48, 50, 64, 77)
T_BATCHES = 7
T_LD = ("odd", "q4")                   # t_ld >= t_rows: not a multiple of 4 (scalar stores) | a multiple of 4
T_EPILOGUES = {"plain": dict(), "bias": dict(bias=True), "rowbias": dict(rowbias=(None, "q4")), "scale": dict(out_scale=0.5),
               "all": dict(bias=True, rowbias=(None, "odd"), out_scale=0.5)}


def t_cases(dtype, epi, ln):
    out = []
    for L in T_ROWS:
        for ld in T_LD:
            for tile in ALL_HINTS:
                e = dict(T_EPILOGUES[epi])
                if e.get("rowbias"):
                    e["rowbias"] = (2 * L + 1, e["rowbias"][1])        # row-bias batches that are not the V^T batches
                out.append(dict(dtype=dtype, M=T_BATCHES * L, N=76 if ln else 70, K=n_K(dtype), tile=tile, ld=ld, trans=L, ln=ln, **e))
    return out


def vt_cases(dtype):
    """merged q | k | v: 128 row-major columns and 40 V columns (a multiple of 8, not of 32), batches of 128 rows"""
    return [dict(dtype=dtype, M=512, N=168, K=n_K(dtype), tile=tile, ld=ld, ln=True, bias=True, vt=(40, 128))
            for tile in (0, 1, 2) for ld in ("q4", "q8")]


# ---- e. split-K ------------------------------------------------------------------------------------------------------------------
# (stages nk, slices S): even | uneven | one trailing empty slice ((S - 1) * ceil(nk / S) >= nk) | more slices than stages
SPLITS = ((8, 2), (8, 4), (10, 3), (10, 4), (10, 6), (3, 5))
SPLIT_N = 128
SPLIT_M_SMALL, SPLIT_M_LARGE = 40, 17003         # 64x64 tiles: 266 x 2 tiles over at most 1024 / S <= 512 blocks - a block walks several
SPLIT_FORMS = {
    "all": dict(bias=True, rowbias=(None, "q4"), residual=1, out_scale=0.5),
    "geglu": dict(bias=True, geglu=True, residual=1, out_scale=0.5),
    "scalar": dict(bias=True, ld="odd"),
    "vt77": dict(bias=True, trans=77, out_scale=0.5),
}


def split_empty(nk, S):
    per = (nk + S - 1) // S
    return (S - 1) * per >= nk


def split_cases(dtype, form, large):
    out = []
    for nk, S in SPLITS:
        K = nk * bk(dtype) - vec(dtype)          # ragged: the last stage is short
        for tile in ((1,) if large else ALL_HINTS):
            e = dict(SPLIT_FORMS[form])
            M = SPLIT_M_LARGE if large else SPLIT_M_SMALL
            if e.get("trans"):
                M = 77 * (221 if large else 1)
            if e.get("rowbias"):
                e["rowbias"] = (M // 3 + 1, e["rowbias"][1])
            out.append(dict(dtype=dtype, M=M, N=SPLIT_N, K=K, tile=tile, split_k=S, **e))
    return out


def planned_empty_slices(limit=None):
    """The planner's own domain searched for shapes whose PLANNED split (split_k = None: emo_gemm_suggest_split_k, as ops.gemm asks)
    leaves a trailing empty slice: few-tile dense shapes over K = nk stages, nk 8 .. 400 (the long-K conv-like shapes nk >= 41
    included), every dtype.  Returns cases (split_k=None)."""
    from emote_hack_amd import _lib, ops
    lib = _lib.load()
    hits = []
    for dtype in DTYPES:
        for M in (64, 128, 300, 640, 1536, 2048):
            for N in (64, 128, 320, 640, 1280):
                for nk in range(8, 401):
                    K = nk * bk(dtype)
                    S = lib.emo_gemm_suggest_split_k(M, N, K, ops.dt(dtype), 0, 0)
                    if S > 1 and split_empty(nk, S):
                        hits.append(dict(dtype=dtype, M=M, N=N, K=K, tile=0, split_k=None, bias=True, residual=1, _nk=nk, _S=S))
                        if limit and len(hits) >= limit:
                            return hits
    return hits


# ---- f. GEGLU with a row bias ---------------------------------------------------------------------------------------------------
def geglu_rowbias_cases(dtype):
    base = dict(dtype=dtype, M=N_M, N=192, K=n_K(dtype), geglu=True, bias=True)
    out = []
    for tile in (2, 4):
        out.append(dict(base, tile=tile, rowbias=(256, "q4")))                 # rows_per_batch % BM == 0: in the accumulators
        out.append(dict(base, tile=tile, rowbias=(100, "q4")))                 # epilogue_row, vector branch
        out.append(dict(base, tile=tile, rowbias=(100, "q4"), ld="odd"))       # epilogue_row, scalar branch
        out.append(dict(base, tile=tile, rowbias=(100, "odd")))                # scalar branch by ld_rowbias
    K_long = 10 * bk(dtype)
    out.append(dict(base, K=K_long, tile=2, rowbias=(100, "q4"), split_k=3))   # the split-K epilogue kernel
    out.append(dict(base, K=K_long, tile=2, rowbias=(256, "q4"), split_k=6, ld="odd"))
    return out


def all_tables():
    """(section name, cases) of everything the GPU module launches - the coverage test walks this"""
    out = []
    for dt_ in DTYPES:
        out.append(("k", k_cases(dt_)))
        out.append(("k_ln", k_ln_cases(dt_)))
        for epi in N_EPILOGUES:
            out.append(("n", n_cases(dt_, epi)))
        for epi in N_GEGLU_EPILOGUES:
            out.append(("n_geglu", n_geglu_cases(dt_, epi)))
        for epi in N_LN_EPILOGUES:
            out.append(("n_ln", n_ln_cases(dt_, epi)))
        out.append(("m", m_cases(dt_)))
        out.append(("m_ln", m_ln_cases(dt_)))
        for epi in T_EPILOGUES:
            for ln in (False, True):
                out.append(("t", t_cases(dt_, epi, ln)))
        out.append(("vt", vt_cases(dt_)))
        for form in SPLIT_FORMS:
            for large in (False, True):
                out.append(("split", split_cases(dt_, form, large)))
        out.append(("geglu_rb", geglu_rowbias_cases(dt_)))
    return out
