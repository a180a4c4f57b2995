"""Case tables of the norm sweeps (csrc/norm.hip: GroupNorm in its two-launch, one-launch, coefficient and folded forms, LayerNorm and its
statistics half), shared by tests/test_gpu_norm_sweeps.py (which launches them) and the CPU coverage test in tests/test_host_logic.py
(which asks emo_groupnorm_plan / emo_layernorm_plan what each would launch).  Plain data, no device needed.

A case names its dtype CLASS - "h": the 2-byte types (bf16 and f16, 8 elements per 16-byte vector), "f": f32 (4) - because the launch
geometry depends on the vector width alone.  A GroupNorm case is (N instances of S rows, C channels, G groups) with the plan it was
written for:
  two = (NC column parts, channels per part, row slots per block, nsplit_stats, nsplit_apply, wide)
  one = (ok, groups per slab, channels per slab, threads, rows per thread of the instantiation, row slots)   zeros: does not fit
A LayerNorm case is (M rows, C) with plan = (lanes per row, rows per wavefront, grid, second trip of the grid-stride loop).
The expectations are what gn_geom / gn1_geom / ln_geom gave when a case was added; a retuning that moves a case to another arm fails
the host test instead of quietly sweeping something else.  Every tensor stays at or below about 50 MB."""
import torch

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
CLASS_DTYPES = {"h": (torch.bfloat16, torch.float16), "f": (torch.float32,)}
GN_THREADS, GN_MAXG, GN_MAXJ = 256, 128, 3          # csrc/norm.hip: threads of a two-launch block, groups, column vectors per thread
GNF_MAXC = 2560                                     # widest row of emo_groupnorm_fold_linear
LN_MAXV, LN_MAXGRID = 5, 4096                       # vectors per lane of a LayerNorm row, blocks of 4 wavefronts per launch


def vec(cls):
    return 8 if cls == "h" else 4


def cls_of(dtype):
    return "f" if dtype == torch.float32 else "h"


def gn(name, cls, N, S, C, G, two, one):
    return dict(name=name, cls=cls, N=N, S=S, C=C, G=G, two=two, one=one)


def ln(cls, M, C, plan):
    return dict(cls=cls, M=M, C=C, plan=plan)


def gn_id(c):
    return f"{c['name']}-{c['cls']}-N{c['N']}-S{c['S']}-C{c['C']}-G{c['G']}"


def ln_id(c):
    return f"{c['cls']}-M{c['M']}-C{c['C']}"


def chunking(S, nsplit):
    """(rows per chunk, chunks that hold rows) of S rows cut into nsplit chunks the way both passes cut them"""
    rows = -(-S // nsplit)
    return rows, -(-S // rows)


def gn_arms(c):
    """the arms of the two-launch kernels a case reaches, derived from its EXPECTED plan"""
    NC, Cp, RP, ns, na, wide = c["two"]
    V, S, cpg = vec(c["cls"]), c["S"], c["C"] // c["G"]
    arms = {f"NC{NC}", "wide" if wide else "narrow"}
    rows_s, live_s = chunking(S, ns)
    rows_a, live_a = chunking(S, na)
    if wide:
        arms.add(f"wide_j{-(-(Cp // V) // GN_THREADS)}")            # column vectors of thread 0
        if (Cp // V) % GN_THREADS:
            arms.add("wide_ragged")                                   # the last vector of some threads only
    else:
        if GN_THREADS % (Cp // V):
            arms.add("idle_threads")
        k = -(-rows_s // RP)                                          # rows of row slot 0 in a full statistics chunk
        arms.add("stats_tail_only" if k < 8 else "stats_unroll8_tail" if k % 8 else "stats_unroll8")
        k = -(-rows_a // RP)
        arms.add("apply_tail_only" if k < 4 else "apply_pipe4_tail" if k % 4 else "apply_pipe4")
    if ns < na:
        arms.add("split_mismatch")
    if live_s < ns:
        arms.add("empty_stats_chunk")
    if live_a < na:
        arms.add("empty_apply_chunk")
    if c["G"] == GN_MAXG:
        arms.add("G128")
    if c["G"] == 1:
        arms.add("G1")
    if S == 1:
        arms.add("S1")
    if cpg < V:
        arms.add("group_narrower_than_vector")
    if cpg % V and V % cpg:
        arms.add("vector_straddles_groups")
    if cpg == 1 and S == 1:
        arms.add("count1")
    return arms


def gn_rerun_as_views(c):
    """the cases run a second time on column views of wider buffers and in place: wide, NC > 1, split-mismatch and empty-chunk ones"""
    return bool(gn_arms(c) & {"wide", "NC2", "NC4", "split_mismatch", "empty_stats_chunk", "empty_apply_chunk"})


def gn_max_chunk_elems(c):
    """elements behind one f32 partial (one group's share of one statistics chunk)"""
    return chunking(c["S"], c["two"][3])[0] * (c["C"] // c["G"])


# ---- GroupNorm: the two-launch arms, the group extremes, the fold's widths and the two rarest one-launch instantiations ------------
GN_TWO = [
    gn("wide257", "h", 2, 37, 2056, 8, two=(1, 2056, 1, 10, 10, 1), one=(0, 0, 0, 0, 0, 0)),
    gn("wide257", "f", 2, 37, 1028, 4, two=(1, 1028, 1, 10, 10, 1), one=(0, 0, 0, 0, 0, 0)),
    gn("wide3", "h", 2, 37, 6144, 3, two=(1, 6144, 1, 10, 10, 1), one=(0, 0, 0, 0, 0, 0)),
    gn("wide3", "f", 2, 37, 3072, 3, two=(1, 3072, 1, 10, 10, 1), one=(0, 0, 0, 0, 0, 0)),
    gn("nc2_wide", "h", 2, 37, 6144, 2, two=(2, 3072, 1, 10, 10, 1), one=(0, 0, 0, 0, 0, 0)),
    gn("nc2_wide", "f", 2, 37, 3072, 2, two=(2, 1536, 1, 10, 10, 1), one=(0, 0, 0, 0, 0, 0)),
    gn("nc4", "h", 2, 37, 6144, 32, two=(4, 1536, 1, 10, 10, 0), one=(1, 1, 192, 256, 4, 10)),
    gn("nc4", "f", 2, 37, 3072, 32, two=(4, 768, 1, 10, 10, 0), one=(1, 1, 96, 256, 4, 10)),
    gn("nc2_at_256", "h", 2, 37, 4096, 2, two=(2, 2048, 1, 10, 10, 0), one=(0, 0, 0, 0, 0, 0)),
    gn("nc2_at_256", "f", 2, 37, 2048, 2, two=(2, 1024, 1, 10, 10, 0), one=(0, 0, 0, 0, 0, 0)),
    gn("split", "h", 1, 4112, 2048, 32, two=(1, 2048, 1, 256, 257, 0), one=(0, 0, 0, 0, 0, 0)),
    gn("split", "f", 1, 4112, 2048, 32, two=(2, 1024, 1, 256, 257, 0), one=(0, 0, 0, 0, 0, 0)),
    gn("empty_apply", "h", 2, 8604, 1032, 8, two=(1, 1032, 1, 256, 512, 0), one=(0, 0, 0, 0, 0, 0)),
    gn("empty_apply", "f", 2, 8604, 516, 4, two=(1, 516, 1, 256, 512, 0), one=(0, 0, 0, 0, 0, 0)),
    gn("unroll8", "h", 32, 4100, 64, 8, two=(1, 64, 32, 9, 9, 0), one=(0, 0, 0, 0, 0, 0)),
    gn("unroll8", "f", 32, 4100, 32, 8, two=(1, 32, 32, 9, 9, 0), one=(1, 1, 4, 1024, 8, 1024)),
    gn("idle", "h", 2, 100, 320, 32, two=(1, 320, 6, 5, 5, 0), one=(0, 0, 0, 0, 0, 0)),
    gn("idle", "f", 2, 100, 160, 32, two=(1, 160, 6, 5, 5, 0), one=(0, 0, 0, 0, 0, 0)),
    gn("g128_c1", "h", 3, 33, 128, 128, two=(1, 128, 16, 1, 1, 0), one=(1, 8, 8, 256, 2, 256)),
    gn("g128_c1", "f", 3, 33, 128, 128, two=(1, 128, 8, 2, 2, 0), one=(1, 4, 4, 256, 2, 256)),
    gn("g128_c2", "h", 3, 33, 256, 128, two=(1, 256, 8, 2, 2, 0), one=(1, 4, 8, 256, 2, 256)),
    gn("g128_c2", "f", 3, 33, 256, 128, two=(1, 256, 4, 3, 3, 0), one=(1, 2, 4, 256, 2, 256)),
    gn("g1", "h", 3, 33, 64, 1, two=(1, 64, 32, 1, 1, 0), one=(0, 0, 0, 0, 0, 0)),
    gn("g1", "f", 3, 33, 64, 1, two=(1, 64, 16, 1, 1, 0), one=(0, 0, 0, 0, 0, 0)),
    gn("s1", "h", 5, 1, 320, 32, two=(1, 320, 6, 1, 1, 0), one=(1, 4, 40, 256, 2, 51)),
    gn("s1", "f", 5, 1, 320, 32, two=(1, 320, 3, 1, 1, 0), one=(1, 2, 20, 256, 2, 51)),
    gn("count1", "h", 2, 1, 128, 128, two=(1, 128, 16, 1, 1, 0), one=(1, 8, 8, 256, 2, 256)),
    gn("count1", "f", 2, 1, 128, 128, two=(1, 128, 8, 1, 1, 0), one=(1, 4, 4, 256, 2, 256)),
    gn("straddle", "h", 3, 33, 96, 16, two=(1, 96, 21, 1, 1, 0), one=(0, 0, 0, 0, 0, 0)),
    gn("straddle", "f", 3, 33, 96, 16, two=(1, 96, 10, 1, 1, 0), one=(0, 0, 0, 0, 0, 0)),
    gn("fold_2560", "h", 2, 50, 2560, 32, two=(2, 1280, 1, 13, 13, 0), one=(1, 1, 80, 256, 2, 25)),
    gn("fold_2560", "f", 2, 50, 2560, 32, two=(4, 640, 1, 13, 13, 0), one=(1, 1, 80, 512, 2, 25)),
    gn("fold_2064", "h", 2, 50, 2064, 16, two=(2, 1032, 1, 13, 13, 0), one=(0, 0, 0, 0, 0, 0)),
    gn("fold_2064", "f", 2, 50, 2064, 16, two=(4, 516, 1, 13, 13, 0), one=(0, 0, 0, 0, 0, 0)),
    gn("fold_2560_gemm", "h", 2, 256, 2560, 32, two=(2, 1280, 1, 64, 64, 0), one=(1, 1, 80, 1024, 4, 102)),
    gn("fold_2560_gemm", "f", 2, 256, 2560, 32, two=(4, 640, 1, 32, 32, 0), one=(1, 1, 80, 1024, 8, 51)),
    gn("fold_2064_gemm", "h", 2, 256, 2064, 16, two=(2, 1032, 1, 64, 64, 0), one=(0, 0, 0, 0, 0, 0)),
    gn("fold_2064_gemm", "f", 2, 256, 2064, 16, two=(4, 516, 1, 32, 32, 0), one=(0, 0, 0, 0, 0, 0)),
    gn("r16", "f", 2, 1633, 320, 32, two=(1, 320, 3, 137, 137, 0), one=(1, 2, 20, 1024, 16, 204)),
    gn("r8", "h", 4, 817, 320, 32, two=(1, 320, 6, 35, 35, 0), one=(1, 4, 40, 1024, 8, 204)),
]

# ---- GroupNorm in one launch: the smallest tensor of every (threads, rows per thread, groups per slab) gn1_geom produces over
# G in {1, 2, 3, 4, 8, 16, 32, 64, 128}, 1 .. 64 channels per group (and 80 .. 2048 in steps of the workload), S < 4200, at 16 or more elements
# per group (fewer belong to the degenerate statistics, which have a test of their own).  16 rows per
# thread need more than 32 K elements per block in the 2-byte types: f32 only.
GN_ONE = [
    gn("one_256_r2_g1", "f", 32, 4, 4, 1, two=(1, 4, 256, 1, 1, 0), one=(1, 1, 4, 256, 2, 256)),
    gn("one_256_r2_g2", "f", 32, 8, 4, 2, two=(1, 4, 256, 1, 1, 0), one=(1, 2, 4, 256, 2, 256)),
    gn("one_256_r2_g4", "f", 32, 16, 4, 4, two=(1, 4, 256, 1, 1, 0), one=(1, 4, 4, 256, 2, 256)),
    gn("one_256_r4_g1", "f", 32, 3, 640, 1, two=(1, 640, 1, 1, 1, 0), one=(1, 1, 640, 256, 4, 1)),
    gn("one_256_r4_g2", "f", 32, 17, 116, 2, two=(1, 116, 8, 1, 1, 0), one=(1, 2, 116, 256, 4, 8)),
    gn("one_256_r4_g4", "f", 32, 11, 172, 4, two=(1, 172, 5, 1, 1, 0), one=(1, 4, 172, 256, 4, 5)),
    gn("one_512_r2_g1", "f", 32, 5, 640, 1, two=(1, 640, 1, 2, 2, 0), one=(1, 1, 640, 512, 2, 3)),
    gn("one_512_r2_g2", "f", 32, 33, 116, 2, two=(1, 116, 8, 2, 2, 0), one=(1, 2, 116, 512, 2, 17)),
    gn("one_512_r2_g4", "f", 32, 17, 212, 4, two=(1, 212, 4, 2, 2, 0), one=(1, 4, 212, 512, 2, 9)),
    gn("one_512_r4_g1", "f", 32, 25, 160, 1, two=(1, 160, 6, 2, 2, 0), one=(1, 1, 160, 512, 4, 12)),
    gn("one_512_r4_g2", "f", 32, 37, 108, 2, two=(1, 108, 9, 2, 2, 0), one=(1, 2, 108, 512, 4, 18)),
    gn("one_512_r4_g4", "f", 32, 17, 228, 4, two=(1, 228, 4, 2, 2, 0), one=(1, 4, 228, 512, 4, 8)),
    gn("one_1024_r2_g1", "f", 32, 49, 160, 1, two=(1, 160, 6, 3, 3, 0), one=(1, 1, 160, 1024, 2, 25)),
    gn("one_1024_r2_g2", "f", 32, 73, 108, 2, two=(1, 108, 9, 3, 3, 0), one=(1, 2, 108, 1024, 2, 37)),
    gn("one_1024_r2_g4", "f", 32, 33, 228, 4, two=(1, 228, 4, 3, 3, 0), one=(1, 4, 228, 1024, 2, 17)),
    gn("one_1024_r4_g1", "f", 32, 25, 320, 1, two=(1, 320, 3, 3, 3, 0), one=(1, 1, 320, 1024, 4, 12)),
    gn("one_1024_r4_g2", "f", 32, 81, 100, 2, two=(1, 100, 10, 3, 3, 0), one=(1, 2, 100, 1024, 4, 40)),
    gn("one_1024_r4_g4", "f", 32, 35, 228, 4, two=(1, 228, 4, 3, 3, 0), one=(1, 4, 228, 1024, 4, 17)),
    gn("one_1024_r8_g1", "f", 32, 49, 320, 1, two=(1, 320, 3, 5, 5, 0), one=(1, 1, 320, 1024, 8, 12)),
    gn("one_1024_r8_g2", "f", 32, 149, 108, 2, two=(1, 108, 9, 5, 5, 0), one=(1, 2, 108, 1024, 8, 37)),
    gn("one_1024_r8_g4", "f", 32, 69, 228, 4, two=(1, 228, 4, 5, 5, 0), one=(1, 4, 228, 1024, 8, 17)),
    gn("one_1024_r16_g1", "f", 32, 97, 320, 1, two=(1, 320, 3, 9, 9, 0), one=(1, 1, 320, 1024, 16, 12)),
    gn("one_1024_r16_g2", "f", 32, 297, 108, 2, two=(1, 108, 9, 9, 9, 0), one=(1, 2, 108, 1024, 16, 37)),
    gn("one_1024_r16_g4", "f", 32, 137, 228, 4, two=(1, 228, 4, 9, 9, 0), one=(1, 4, 228, 1024, 16, 17)),
    gn("one_256_r2_g1", "h", 32, 2, 8, 1, two=(1, 8, 256, 1, 1, 0), one=(1, 1, 8, 256, 2, 256)),
    gn("one_256_r2_g2", "h", 32, 4, 8, 2, two=(1, 8, 256, 1, 1, 0), one=(1, 2, 8, 256, 2, 256)),
    gn("one_256_r2_g4", "h", 32, 8, 8, 4, two=(1, 8, 256, 1, 1, 0), one=(1, 4, 8, 256, 2, 256)),
    gn("one_256_r2_g8", "h", 32, 16, 8, 8, two=(1, 8, 256, 1, 1, 0), one=(1, 8, 8, 256, 2, 256)),
    gn("one_256_r4_g1", "h", 32, 3, 1280, 1, two=(1, 1280, 1, 1, 1, 0), one=(1, 1, 1280, 256, 4, 1)),
    gn("one_256_r4_g2", "h", 32, 39, 104, 2, two=(1, 104, 19, 1, 1, 0), one=(1, 2, 104, 256, 4, 19)),
    gn("one_256_r4_g4", "h", 32, 17, 232, 4, two=(1, 232, 8, 1, 1, 0), one=(1, 4, 232, 256, 4, 8)),
    gn("one_256_r4_g8", "h", 32, 11, 344, 8, two=(1, 344, 5, 1, 1, 0), one=(1, 8, 344, 256, 4, 5)),
    gn("one_512_r2_g1", "h", 32, 5, 1280, 1, two=(1, 1280, 1, 2, 2, 0), one=(1, 1, 1280, 512, 2, 3)),
    gn("one_512_r2_g2", "h", 32, 77, 104, 2, two=(1, 104, 19, 2, 2, 0), one=(1, 2, 104, 512, 2, 39)),
    gn("one_512_r2_g4", "h", 32, 33, 232, 4, two=(1, 232, 8, 2, 2, 0), one=(1, 4, 232, 512, 2, 17)),
    gn("one_512_r2_g8", "h", 32, 17, 424, 8, two=(1, 424, 4, 2, 2, 0), one=(1, 8, 424, 512, 2, 9)),
    gn("one_512_r4_g1", "h", 32, 25, 320, 1, two=(1, 320, 6, 2, 2, 0), one=(1, 1, 320, 512, 4, 12)),
    gn("one_512_r4_g2", "h", 32, 113, 72, 2, two=(1, 72, 28, 2, 2, 0), one=(1, 2, 72, 512, 4, 56)),
    gn("one_512_r4_g4", "h", 32, 37, 216, 4, two=(1, 216, 9, 2, 2, 0), one=(1, 4, 216, 512, 4, 18)),
    gn("one_512_r4_g8", "h", 32, 17, 456, 8, two=(1, 456, 4, 2, 2, 0), one=(1, 8, 456, 512, 4, 8)),
    gn("one_1024_r2_g1", "h", 32, 49, 320, 1, two=(1, 320, 6, 3, 3, 0), one=(1, 1, 320, 1024, 2, 25)),
    gn("one_1024_r2_g2", "h", 32, 225, 72, 2, two=(1, 72, 28, 3, 3, 0), one=(1, 2, 72, 1024, 2, 113)),
    gn("one_1024_r2_g4", "h", 32, 73, 216, 4, two=(1, 216, 9, 3, 3, 0), one=(1, 4, 216, 1024, 2, 37)),
    gn("one_1024_r2_g8", "h", 32, 33, 456, 8, two=(1, 456, 4, 3, 3, 0), one=(1, 8, 456, 1024, 2, 17)),
    gn("one_1024_r4_g1", "h", 32, 25, 640, 1, two=(1, 640, 3, 3, 3, 0), one=(1, 1, 640, 1024, 4, 12)),
    gn("one_1024_r4_g2", "h", 32, 157, 104, 2, two=(1, 104, 19, 3, 3, 0), one=(1, 2, 104, 1024, 4, 78)),
    gn("one_1024_r4_g4", "h", 32, 81, 200, 4, two=(1, 200, 10, 3, 3, 0), one=(1, 4, 200, 1024, 4, 40)),
    gn("one_1024_r4_g8", "h", 32, 35, 456, 8, two=(1, 456, 4, 3, 3, 0), one=(1, 8, 456, 1024, 4, 17)),
    gn("one_1024_r8_g1", "h", 32, 49, 640, 1, two=(1, 640, 3, 5, 5, 0), one=(1, 1, 640, 1024, 8, 12)),
    gn("one_1024_r8_g2", "h", 32, 313, 104, 2, two=(1, 104, 19, 5, 5, 0), one=(1, 2, 104, 1024, 8, 78)),
    gn("one_1024_r8_g4", "h", 32, 149, 216, 4, two=(1, 216, 9, 5, 5, 0), one=(1, 4, 216, 1024, 8, 37)),
    gn("one_1024_r8_g8", "h", 32, 69, 456, 8, two=(1, 456, 4, 5, 5, 0), one=(1, 8, 456, 1024, 8, 17)),
]

# ---- LayerNorm: every lanes-per-row choice in both vector widths at its narrowest and its widest row, M in {1, a wavefront's rows - 1
# and + 1}, and at the narrowest row one M past 4096 blocks (the grid-stride loop's second trip, with a partly filled last wavefront)
LN = [
    ln("h", 1, 8, plan=(1, 64, 1, 0)),
    ln("h", 63, 8, plan=(1, 64, 1, 0)),
    ln("h", 65, 8, plan=(1, 64, 1, 0)),
    ln("h", 1, 40, plan=(1, 64, 1, 0)),
    ln("h", 63, 40, plan=(1, 64, 1, 0)),
    ln("h", 65, 40, plan=(1, 64, 1, 0)),
    ln("h", 1048641, 8, plan=(1, 64, 4096, 1)),
    ln("h", 1, 48, plan=(2, 32, 1, 0)),
    ln("h", 31, 48, plan=(2, 32, 1, 0)),
    ln("h", 33, 48, plan=(2, 32, 1, 0)),
    ln("h", 1, 80, plan=(2, 32, 1, 0)),
    ln("h", 31, 80, plan=(2, 32, 1, 0)),
    ln("h", 33, 80, plan=(2, 32, 1, 0)),
    ln("h", 524321, 48, plan=(2, 32, 4096, 1)),
    ln("h", 1, 88, plan=(4, 16, 1, 0)),
    ln("h", 15, 88, plan=(4, 16, 1, 0)),
    ln("h", 17, 88, plan=(4, 16, 1, 0)),
    ln("h", 1, 160, plan=(4, 16, 1, 0)),
    ln("h", 15, 160, plan=(4, 16, 1, 0)),
    ln("h", 17, 160, plan=(4, 16, 1, 0)),
    ln("h", 262161, 88, plan=(4, 16, 4096, 1)),
    ln("h", 1, 168, plan=(8, 8, 1, 0)),
    ln("h", 7, 168, plan=(8, 8, 1, 0)),
    ln("h", 9, 168, plan=(8, 8, 1, 0)),
    ln("h", 1, 320, plan=(8, 8, 1, 0)),
    ln("h", 7, 320, plan=(8, 8, 1, 0)),
    ln("h", 9, 320, plan=(8, 8, 1, 0)),
    ln("h", 131081, 168, plan=(8, 8, 4096, 1)),
    ln("h", 1, 328, plan=(16, 4, 1, 0)),
    ln("h", 3, 328, plan=(16, 4, 1, 0)),
    ln("h", 5, 328, plan=(16, 4, 1, 0)),
    ln("h", 1, 640, plan=(16, 4, 1, 0)),
    ln("h", 3, 640, plan=(16, 4, 1, 0)),
    ln("h", 5, 640, plan=(16, 4, 1, 0)),
    ln("h", 65541, 328, plan=(16, 4, 4096, 1)),
    ln("h", 1, 648, plan=(32, 2, 1, 0)),
    ln("h", 3, 648, plan=(32, 2, 1, 0)),
    ln("h", 1, 1280, plan=(32, 2, 1, 0)),
    ln("h", 3, 1280, plan=(32, 2, 1, 0)),
    ln("h", 32771, 648, plan=(32, 2, 4096, 1)),
    ln("h", 1, 1288, plan=(64, 1, 1, 0)),
    ln("h", 2, 1288, plan=(64, 1, 1, 0)),
    ln("h", 1, 2560, plan=(64, 1, 1, 0)),
    ln("h", 2, 2560, plan=(64, 1, 1, 0)),
    ln("h", 16386, 1288, plan=(64, 1, 4096, 1)),
    ln("f", 1, 4, plan=(1, 64, 1, 0)),
    ln("f", 63, 4, plan=(1, 64, 1, 0)),
    ln("f", 65, 4, plan=(1, 64, 1, 0)),
    ln("f", 1, 20, plan=(1, 64, 1, 0)),
    ln("f", 63, 20, plan=(1, 64, 1, 0)),
    ln("f", 65, 20, plan=(1, 64, 1, 0)),
    ln("f", 1048641, 4, plan=(1, 64, 4096, 1)),
    ln("f", 1, 24, plan=(2, 32, 1, 0)),
    ln("f", 31, 24, plan=(2, 32, 1, 0)),
    ln("f", 33, 24, plan=(2, 32, 1, 0)),
    ln("f", 1, 40, plan=(2, 32, 1, 0)),
    ln("f", 31, 40, plan=(2, 32, 1, 0)),
    ln("f", 33, 40, plan=(2, 32, 1, 0)),
    ln("f", 524321, 24, plan=(2, 32, 4096, 1)),
    ln("f", 1, 44, plan=(4, 16, 1, 0)),
    ln("f", 15, 44, plan=(4, 16, 1, 0)),
    ln("f", 17, 44, plan=(4, 16, 1, 0)),
    ln("f", 1, 80, plan=(4, 16, 1, 0)),
    ln("f", 15, 80, plan=(4, 16, 1, 0)),
    ln("f", 17, 80, plan=(4, 16, 1, 0)),
    ln("f", 262161, 44, plan=(4, 16, 4096, 1)),
    ln("f", 1, 84, plan=(8, 8, 1, 0)),
    ln("f", 7, 84, plan=(8, 8, 1, 0)),
    ln("f", 9, 84, plan=(8, 8, 1, 0)),
    ln("f", 1, 160, plan=(8, 8, 1, 0)),
    ln("f", 7, 160, plan=(8, 8, 1, 0)),
    ln("f", 9, 160, plan=(8, 8, 1, 0)),
    ln("f", 131081, 84, plan=(8, 8, 4096, 1)),
    ln("f", 1, 164, plan=(16, 4, 1, 0)),
    ln("f", 3, 164, plan=(16, 4, 1, 0)),
    ln("f", 5, 164, plan=(16, 4, 1, 0)),
    ln("f", 1, 320, plan=(16, 4, 1, 0)),
    ln("f", 3, 320, plan=(16, 4, 1, 0)),
    ln("f", 5, 320, plan=(16, 4, 1, 0)),
    ln("f", 65541, 164, plan=(16, 4, 4096, 1)),
    ln("f", 1, 324, plan=(32, 2, 1, 0)),
    ln("f", 3, 324, plan=(32, 2, 1, 0)),
    ln("f", 1, 640, plan=(32, 2, 1, 0)),
    ln("f", 3, 640, plan=(32, 2, 1, 0)),
    ln("f", 32771, 324, plan=(32, 2, 4096, 1)),
    ln("f", 1, 644, plan=(64, 1, 1, 0)),
    ln("f", 2, 644, plan=(64, 1, 1, 0)),
    ln("f", 1, 1280, plan=(64, 1, 1, 0)),
    ln("f", 2, 1280, plan=(64, 1, 1, 0)),
    ln("f", 16386, 644, plan=(64, 1, 4096, 1)),
]

GN = GN_TWO + GN_ONE

# what the tables must reach between them (tests/test_host_logic.py asserts the equality, so a deleted case fails there)
GN_TWO_ARMS = {"narrow", "wide", "wide_j2", "wide_j3", "wide_ragged", "NC1", "NC2", "NC4", "idle_threads", "stats_tail_only", "stats_unroll8", "stats_unroll8_tail",
               "apply_tail_only", "apply_pipe4", "apply_pipe4_tail", "split_mismatch", "empty_stats_chunk", "empty_apply_chunk", "G128", "G1", "S1", "count1",
               "group_narrower_than_vector", "vector_straddles_groups"}
GN_ONE_SHAPES = {"f": {(nt, r, g) for nt, rs in ((256, (2, 4)), (512, (2, 4)), (1024, (2, 4, 8, 16))) for r in rs for g in (1, 2, 4)},
                 "h": {(nt, r, g) for nt, rs in ((256, (2, 4)), (512, (2, 4)), (1024, (2, 4, 8))) for r in rs for g in (1, 2, 4, 8)}}
LN_LPRS = (1, 2, 4, 8, 16, 32, 64)

# shapes every GroupNorm entry refuses: (N, S, C, G, class)
GN_REFUSED = [(2, 37, 129 * 8, 129, "h"), (2, 37, 129 * 4, 129, "f"),          # G = 129
              (2, 37, 769 * 8, 1, "h"), (2, 37, 769 * 4, 1, "f"),              # more than 768 column vectors
              (2, 37, 320, 33, "h"), (2, 37, 320, 33, "f"),                    # C % G
              (2, 37, 324, 4, "h"), (2, 37, 322, 2, "f")]                      # C % vector width
