"""Case tables of the halo-reuse 3x3 conv sweeps (csrc/conv_halo_impl.h), shared by tests/test_gpu_conv_halo_sweeps.py (which launches
them) and the CPU coverage test in tests/test_host_logic.py (which asks emo_conv3x3_halo_plan what each would launch).  Plain data, no
device needed.

A case is a dict without a dtype (every case runs in every dtype): ph (patch height, pinned through emo_gemm_params.tile), tile (the
further tile bits: 4 single launch | 8 keep the 64-column tail | 16 force the 192-column blocks), n frames of H x W SOURCE pixels
(ups: nearest x2 inside the loader, the patch grid lives on the doubled frame), chunks (Cin in 128-byte channel chunks: 64 elements
in the 2-byte types, 32 in f32), N, gn (the GroupNorm fold), main / tail (the block widths the case expects of its launches, 0 = no
such launch), many (the launches in which every block must walk at least two tiles and some three) and the epilogue keys of
DEFAULTS."""
import torch

from tests.gemm_sweep_cases import DTYPES, bk, ld_of, vec      # noqa: F401  (re-exported)

GRID = {8: 512, 16: 256}                # persistent blocks of a launch: min(tiles, GRID[ph])
PERIOD = 7                              # distinct frames of a many-tile run: coprime with both grids and the 8-way tile interleave

DEFAULTS = dict(tile=0, ups=False, gn=False, main=128, tail=0, many=(),
                lda_pad=0,              # the input is the left part of a buffer lda_pad elements wider
                ldc=None, ldr=None,     # leading-dimension class of the output / residual view ("q8" | "q4"); None = contiguous
                bias=True, rowbias=False,
                residual=0,             # 0 none | 1 its own buffer | 2 the output (in place)
                out_scale=1.0)


def full(case):
    c = dict(DEFAULTS)
    c.update(case)
    return c


def frame(case):
    """(He, We): the frame the patch grid lives on"""
    c = full(case)
    return (2 * c["H"], 2 * c["W"]) if c["ups"] else (c["H"], c["W"])


def tile_bits(case):
    c = full(case)
    return (1 if c["ph"] == 8 else 2) | c["tile"]


C0 = 16                                 # first output column inside a wider output buffer: C stays 16-byte aligned in every dtype


def geometry(case, dtype):
    """Cin, lda, ldc, ldr of a case in a dtype (ldc counts the C0 columns in front of the view)"""
    c = full(case)
    cin = c["chunks"] * bk(dtype)
    return dict(Cin=cin, lda=cin + c["lda_pad"], ldc=ld_of(c["ldc"], C0 + c["N"]) if c["ldc"] else c["N"],
                ldr=ld_of(c["ldr"], c["N"]) if c["ldr"] else c["N"])


def plan_kwargs(case, dtype):
    c, g = full(case), geometry(case, dtype)
    He, We = frame(case)
    kw = dict(dtype=dtype, n_img=c["n"], H=c["H"], W=c["W"], Cin=g["Cin"], N=c["N"], upsample2x=c["ups"], lda=g["lda"], ldc=g["ldc"],
              bias=c["bias"], out_scale=c["out_scale"], gn=c["gn"], imgs_per_inst=c.get("imgs_per_inst", 1), tile=tile_bits(case))
    if c["rowbias"]:
        kw.update(rowbias=True, rows_per_batch=He * We)
    if c["residual"] == 1:
        kw.update(residual=True, ldr=g["ldr"])
    elif c["residual"] == 2:
        kw.update(inplace=True)
    return kw


def plan(case, dtype):
    from emote_hack_amd import ops
    return ops.conv_halo_plan(**plan_kwargs(case, dtype))


def tile_of(i, tiles_all):
    """the tile the i-th step of the persistent walk computes (conv_halo_impl.h tile_of): tiles dealt out in 8 contiguous runs"""
    qn, rn, x, idx = tiles_all >> 3, tiles_all & 7, i & 7, i >> 3
    return (x * (qn + 1) if x < rn else rn * (qn + 1) + (x - rn) * qn) + idx


# ---- a. many tiles per block (plain): every block walks at least two tiles, some three -------------------------------------------
# 8-row patches run min(tiles, 512) blocks: 1025 tiles at the least; 16-row patches min(tiles, 256): 513.
MANY = [
    dict(ph=8, N=256, H=8, W=16, n=552, chunks=1, many=("main",)),                              # 128 + 128 columns: 1104 tiles
    dict(ph=8, N=128, H=8, W=16, n=1101, chunks=2, many=("main",)),
    dict(ph=8, N=64, H=8, W=16, n=1103, chunks=3, main=64, many=("main",)),                     # 64-column blocks
    dict(ph=8, N=320, H=16, W=16, n=513, chunks=1, tail=64, many=("main", "tail")),             # 128 + 128, tail 64: 2052 and 1026 tiles
    dict(ph=8, N=128, H=12, W=24, n=257, chunks=1, many=("main",)),                             # ragged: both last patches overlapped
    dict(ph=8, N=128, H=4, W=8, ups=True, n=1101, chunks=1, many=("main",)),                    # 4x8 -> 8x16
    dict(ph=16, N=128, H=16, W=16, n=563, chunks=1, many=("main",)),
    dict(ph=16, N=64, H=16, W=16, n=560, chunks=2, main=64, many=("main",)),
    dict(ph=16, N=192, H=16, W=16, n=565, chunks=1, main=0, tail=192, many=("tail",)),          # 192-column blocks, one launch
    dict(ph=16, N=320, H=16, W=16, n=565, chunks=1, tile=16, tail=192, many=("main", "tail")),  # forced 128 + 192
]
for _c in MANY:
    _c.update(rowbias=True, residual=1)

# ---- b. the GroupNorm fold over many tiles and 3 instances -------------------------------------------------------------------------
GN_INSTANCES = 3
GN_FR = {8: 184, 16: 188}               # frames per instance of the big run (16 x 16 frames: 1104 / 564 patches)
GN_MANY = [dict(ph=ph, N=N, H=16, W=16, n=GN_INSTANCES * GN_FR[ph], imgs_per_inst=GN_FR[ph], chunks=chunks, gn=True,
                main=64 if N == 64 else 128, tail=64 if N == 320 else 0, many=("main", "tail") if N == 320 else ("main",))
           for ph, widths in ((8, (128, 64, 320)), (16, (128, 64))) for N in widths for chunks in (1, 2)]

# ---- c. pad pixels stay zero under the fold: N = 12 (nine taps, padded), 2 frames ------------------------------------------------------
# (a 16-row patch needs a frame of 16 rows: 16 x 16 is its "every pixel of the only patch is on a border" frame, 32 x 32 the one
# with interior patch edges in both directions)
PAD_N = 12
PAD = [dict(ph=ph, N=PAD_N, H=H, W=W, n=2, chunks=chunks, gn=True, bias=False, live=live)
       for ph, frames in ((8, ((8, 16), (16, 32))), (16, ((16, 16), (16, 32), (32, 32))))
       for H, W in frames for chunks, live in ((1, "first"), (2, "first"), (2, "second"))]      # live: the chunk of the tapped channel

# ---- d. impulse: every tap, chunk edge and border (no GN, no bias) -----------------------------------------------------------------------
IMPULSE_N = 36                          # column 4 t + j: tap t of channel c_j, c_j in {0, BK - 1, BK, Cin - 1}
IMPULSE = [dict(ph=ph, N=IMPULSE_N, H=H, W=W, ups=ups, n=2, chunks=2, bias=False)
           for ph, frames in ((8, ((8, 16, False), (9, 17, False), (24, 24, False), (6, 12, True))),
                              (16, ((16, 24, False), (32, 40, False), (8, 12, True))))
           for H, W, ups in frames]


def impulse_channels(dtype):
    BK = bk(dtype)
    return (0, BK - 1, BK, 2 * BK - 1)


# ---- e. 16-row patches and 192-column blocks on ragged frames ------------------------------------------------------------------------------
RAGGED16_FRAMES = ((16, 24), (32, 40), (16, 17))
RAGGED16_N = (128, 132, 192, 320)
# launch shapes of a width that is an odd multiple of 64, by tile bit: (main, tail) block widths at N = 192 and at N = 320
RAGGED16_SHAPES = {4: {192: (192, 0), 320: (128, 0)}, 8: {192: (128, 64), 320: (128, 64)}, 16: {192: (0, 192), 320: (128, 192)}}


def ragged16_case(H, W, N, bit=0):
    main, tail = RAGGED16_SHAPES[bit][N] if bit else ((128, 0) if N in (128, 132) else RAGGED16_SHAPES[16][N])   # (few patches: planned wide)
    return dict(ph=16, N=N, H=H, W=W, n=3, chunks=2, tile=bit, main=main, tail=tail, rowbias=True, residual=1)


RAGGED16 = [ragged16_case(H, W, N, bit) for H, W in RAGGED16_FRAMES for N in RAGGED16_N for bit in ((0, 4, 8, 16) if N in (192, 320) else (0,))]

# ---- f. strides and epilogue paths -------------------------------------------------------------------------------------------------------
EPI_FRAMES = ((16, 32), (12, 24))       # whole (both patch heights, plain and GN) and ragged (8-row patches, plain)
EPI_N = (128, 132)
EPI_FORMS = {
    "wide_in": dict(lda_pad=64),                                             # the input is the left part of a wider buffer
    "out_q8": dict(ldc="q8"),                                                # output as a column view; q4: the row epilogue in the 2-byte types
    "out_q4": dict(ldc="q4"),
    "res_q8": dict(residual=1, ldr="q8"),
    "res_q4": dict(residual=1, ldr="q4"),
    "scale": dict(out_scale=0.5),
    "scale_res": dict(out_scale=0.5, residual=1),
    "all": dict(lda_pad=64, ldc="q4", residual=1, ldr="q4", out_scale=0.5),
}


def epi_variants(H, W):
    """(patch height, gn) a frame runs in"""
    whole = H % 8 == 0 and W % 16 == 0
    return [(ph, gn) for ph in ((8, 16) if H % 16 == 0 else (8,)) for gn in ((False, True) if whole else (False,))]


def epi_case(H, W, N, ph, gn, form):
    return dict(ph=ph, N=N, H=H, W=W, n=2, chunks=2, gn=gn, imgs_per_inst=1, rowbias=True, **EPI_FORMS[form])


EPI = [epi_case(H, W, N, ph, gn, form) for H, W in EPI_FRAMES for N in EPI_N for ph, gn in epi_variants(H, W) for form in EPI_FORMS]
# the in-place residual: served on whole frames (plain and GN)
INPLACE = [dict(ph=ph, N=N, H=16, W=32, n=2, chunks=2, gn=gn, imgs_per_inst=1, rowbias=True, residual=2)
           for N in EPI_N for ph, gn in epi_variants(16, 32)]
# ... and NOT on ragged ones (two blocks store the overlapped pixels: the second would add the residual to the first one's sum)
INPLACE_RAGGED = [dict(ph=8, N=N, H=12, W=24, n=2, chunks=2, rowbias=True, residual=2) for N in EPI_N]


def all_tables():
    """(section name, cases) of everything the GPU module launches on the halo kernel - the coverage test walks this"""
    return [("many", MANY), ("gn_many", GN_MANY), ("pad", PAD), ("impulse", IMPULSE), ("ragged16", RAGGED16), ("epi", EPI),
            ("inplace", INPLACE)]
