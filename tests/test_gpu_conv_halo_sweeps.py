"""GPU sweeps of the halo-reuse 3x3 conv (csrc/conv_halo_impl.h conv3x3_halo_kernel; launch decisions: csrc/gemm.hip plan_halo) over
what its random-input tests in tests/test_gpu_kernels.py leave out: blocks that walk several tiles (tile_of, the loader stream and
the halo-buffer parity across a tile boundary, the GroupNorm fold's per-tile coefficient row), pad pixels under the fold, every tap /
chunk edge / border on exact data, 16-row patches and 192-column blocks on ragged frames, strided operands and the row epilogue.

The cases are the tables of tests/halo_sweep_cases.py; tests/test_host_logic.py checks on the CPU (emo_conv3x3_halo_plan) that each
runs on the block shape it names and that together they reach every instantiation.  Exact groups compare bits (torch.equal): per
output element the kernel's arithmetic and its order are fixed - which block computes a tile, and how many tiles it walked before,
must not show.  The other groups compare with F.conv2d in f32 on the CPU at the tolerances of tests/test_gpu_kernels.py."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from emote_hack_amd.synth import seeded_randn
from tests import halo_sweep_cases as S
from tests.test_gpu_conv_loader import pack_w, to_rows
from tests.test_gpu_kernels import DEV, DTYPES, TOL, close, ops, q      # noqa: F401  (TOL: the only tolerances used here)

pytestmark = pytest.mark.gpu

P = S.PERIOD
SENTINEL = 3.0                          # fills the buffers around a strided view (exact in every dtype)


def name_of(case):
    c = S.full(case)
    bits = [f"ph{c['ph']}", f"N{c['N']}", f"{c['n']}x{c['H']}x{c['W']}" + ("up" if c["ups"] else ""), f"c{c['chunks']}"]
    bits += [f"t{c['tile']}"] if c["tile"] else []
    bits += ["gn"] if c["gn"] else []
    bits += [f"{k}{c[k]}" for k in ("live", "lda_pad", "ldc", "ldr") if c.get(k)]
    bits += [f"res{c['residual']}"] if c["residual"] else []
    bits += ["half"] if c["out_scale"] != 1.0 else []
    return "-".join(bits)


def cases_of(table):
    return pytest.mark.parametrize("case", table, ids=[name_of(c) for c in table])


def dev(t, dtype):
    return t.to(DEV).to(dtype)


def up2(x, ups):
    return F.interpolate(x, scale_factor=2.0, mode="nearest") if ups else x


def out_rows(y):
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


def coef_table(scale, shift):
    """(instances, Cin) scales and shifts -> the f32 (instances, 2 * Cin) table of emo_gemm_params.gn_coef: per channel pair
    (scale, scale, shift, shift)"""
    n, cin = scale.shape
    return torch.stack([scale.reshape(n, cin // 2, 2), shift.reshape(n, cin // 2, 2)], 2).reshape(n, 2 * cin).contiguous()


def gn_ref(x, scale, shift, inst_of_frame, silu, dtype):
    """the fold's f32 statement: x * scale + shift per (instance, channel), optional SiLU, rounded to the compute dtype"""
    xn = x * scale[inst_of_frame][:, :, None, None] + shift[inst_of_frame][:, :, None, None]
    return q(F.silu(xn) if silu else xn, dtype)


def repeat_frames(rows, n_small, idx):
    """rows of n_small frames -> the rows of frames idx[0], idx[1], ... (device gather)"""
    return rows.reshape(n_small, -1, rows.shape[1])[idx].reshape(-1, rows.shape[1])


def assert_frames_equal(big, small, src, tiles_per_frame, what):
    """big frame i must hold the bits of small frame src[i]"""
    n = src.numel()
    b = big.reshape(n, -1, big.shape[1])
    s = small.reshape(-1, b.shape[1], small.shape[1])
    assert s.shape[0] == int(src.max()) + 1
    want = s[src]
    if torch.equal(b, want):
        return
    bad = torch.nonzero(~(b == want).flatten(1).all(1)).flatten().tolist()
    cols = torch.nonzero(~(b == want).all(1).all(0)).flatten().tolist()
    worst = float((b.float() - want.float()).abs().max())
    raise AssertionError(f"{what}: {len(bad)} of {n} frames differ from their {s.shape[0]}-frame run (first {bad[:12]}, "
                         f"{tiles_per_frame} row tiles per frame; columns {cols[:4]}..{cols[-1:]}; max |diff| {worst:.3e})")


# ------------------------------------------------------------------------------------------------ a. many tiles per block, exact
@pytest.mark.parametrize("dtype", DTYPES)
@cases_of(S.MANY)
def test_many_tiles_per_block_give_the_bits_of_a_seven_frame_run(dtype, case):
    """Every block of these launches walks two tiles, some three (tests/test_host_logic.py holds the tables to that): tile_of, the
    loader stream running one chunk ahead into the NEXT tile, the halo-buffer parity carried over (odd and even chunk counts), the
    weight descriptor of the next tile, the epilogue staging in the free halo buffer.  Frame i of the big run has the content, row
    bias and residual of frame i % 7 (7 is coprime with the grids and the 8-way tile interleave, so a frame's neighbours in a
    block's walk change all the time): it must hold the BITS the same frame gets in a run of the 7 frames alone - there every block
    computes one tile - and that run must be the f32 conv."""
    o = ops()
    c, g = S.full(case), S.geometry(case, dtype)
    Cin, N, H, W, n, ups = g["Cin"], c["N"], c["H"], c["W"], c["n"], c["ups"]
    He, We = S.frame(case)
    x = q(seeded_randn((P, Cin, H, W), 511), dtype)
    wt, bias = q(seeded_randn((N, Cin, 3, 3), 512) / math.sqrt(9 * Cin), dtype), 0.1 * seeded_randn((N,), 513)
    res, rb = q(seeded_randn((P, N, He, We), 514), dtype), seeded_randn((P, N), 515)
    ref = out_rows(F.conv2d(up2(x, ups), wt, bias, padding=1) + rb[:, :, None, None] + res)
    rows, wp, rrows, rbd, bd = dev(to_rows(x), dtype), dev(pack_w(wt), dtype), dev(to_rows(res), dtype), rb.to(DEV), bias.to(DEV)
    kw = dict(upsample2x=ups, rows_per_batch=He * We, split_k=1, tile=S.tile_bits(case))
    small, _, _ = o.conv3x3(rows, wp, bd, P, H, W, rowbias=rbd, residual=rrows, **kw)
    close(small, ref, dtype)
    src = torch.arange(n, device=DEV) % P
    big, Ho, Wo = o.conv3x3(repeat_frames(rows, P, src), wp, bd, n, H, W, rowbias=rbd[src].contiguous(), residual=repeat_frames(rrows, P, src), **kw)
    assert (Ho, Wo) == (He, We)
    assert_frames_equal(big, small, src, -(-He // c["ph"]) * -(-We // 16), name_of(case))


# ------------------------------------------------------------------------------------------------ b. the GN fold over many tiles
def gn_hand_table(n_inst, cin, seed):
    """coefficients that differ grossly between instances: |scale| about 1, 2, 4 with alternating signs, shifts near -1, 0, 1"""
    sign = 1.0 - 2.0 * ((torch.arange(cin)[None, :] + torch.arange(n_inst)[:, None]) % 2)
    scale = sign * (2.0 ** torch.arange(n_inst))[:, None] * (1 + 0.1 * seeded_randn((n_inst, cin), seed))
    shift = (torch.arange(n_inst) - 1.0)[:, None] + 0.1 * seeded_randn((n_inst, cin), seed + 1)
    return scale.float(), shift.float()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("silu", [True, False])
@cases_of(S.GN_MANY)
def test_groupnorm_fold_many_tiles_and_instances_give_the_bits_of_a_small_run(dtype, silu, case):
    """The fold's cross-tile state: the coefficient row (g_row) of the tile the LOADER is on against the tile being computed, the
    slot validity latched at request time, the first chunk of a block normalised in the prologue and every later one spread over
    the taps.  3 instances with a hand-made table whose rows differ grossly (taking a neighbour's row cannot hide in a tolerance);
    frame i of the big run has content i % 7 and instance i // Fr and must hold the bits of frame (i // Fr) * 7 + i % 7 of a 21-frame
    run with 7 frames per instance - the same table goes to both, so no statistics enter.  The small run is held against the f32
    statement (x * scale + shift, SiLU, rounded to the compute dtype, conv2d with zero padding of the NORMALISED tensor)."""
    o = ops()
    c, g = S.full(case), S.geometry(case, dtype)
    Cin, N, H, W, n, Fr, I = g["Cin"], c["N"], c["H"], c["W"], c["n"], c["imgs_per_inst"], S.GN_INSTANCES
    x = q(seeded_randn((P, Cin, H, W), 521), dtype)
    wt, bias = q(seeded_randn((N, Cin, 3, 3), 522) / math.sqrt(9 * Cin), dtype), 0.1 * seeded_randn((N,), 523)
    scale, shift = gn_hand_table(I, Cin, 524)
    inst_small = torch.arange(I * P) // P
    xs = x.repeat(I, 1, 1, 1)
    ref = out_rows(F.conv2d(gn_ref(xs, scale, shift, inst_small, silu, dtype), wt, bias, padding=1))
    rows, wp, bd, coef = dev(to_rows(x), dtype), dev(pack_w(wt), dtype), bias.to(DEV), coef_table(scale, shift).to(DEV)
    kw = dict(split_k=1, tile=S.tile_bits(case))
    small, _, _ = o.conv3x3(rows.repeat(I, 1), wp, bd, I * P, H, W, gn=(coef, P, silu), **kw)
    close(small, ref, dtype, scale=2.0)
    i = torch.arange(n, device=DEV)
    big, _, _ = o.conv3x3(repeat_frames(rows, P, i % P), wp, bd, n, H, W, gn=(coef, Fr, silu), **kw)
    assert_frames_equal(big, small, (i // Fr) * P + i % P, -(-H // c["ph"]) * -(-W // 16), name_of(case))


# ------------------------------------------------------------------------------------------------ c. pad pixels under the fold
@pytest.mark.parametrize("dtype", DTYPES)
@cases_of(S.PAD)
def test_pad_pixels_stay_zero_under_the_groupnorm_fold(dtype, case):
    """The conv pads the NORMALISED tensor: a pad pixel's slot in the halo must stay 0, not become silu(shift).  Scale 0 and shift 4
    for every channel make the normalised tensor exactly 4 inside the frame whatever x holds; output column t takes tap t of one
    channel with weight 1 - so every output is exactly 4 where the tapped pixel is inside the frame and exactly 0 where it is
    padding, in every dtype.  A frame of one patch has every halo edge on the border; frames of several patches have interior
    patch edges, which must NOT read zero."""
    o = ops()
    c, g = S.full(case), S.geometry(case, dtype)
    Cin, N, H, W, n = g["Cin"], c["N"], c["H"], c["W"], c["n"]
    live = 5 if c["live"] == "first" else Cin - 3
    assert (live >= S.bk(dtype)) == (c["live"] == "second")
    x = q(seeded_randn((n, Cin, H, W), 531), dtype)
    wt = torch.zeros(N, Cin, 3, 3)
    for t in range(9):
        wt[t, live, t // 3, t % 3] = 1.0
    coef = coef_table(torch.zeros(n, Cin), torch.full((n, Cin), 4.0)).to(DEV)
    got, _, _ = o.conv3x3(dev(to_rows(x), dtype), dev(pack_w(wt), dtype), None, n, H, W, gn=(coef, 1, False), split_k=1, tile=S.tile_bits(case))
    inside = F.conv2d(torch.full((n, 1, H, W), 4.0), torch.eye(9).reshape(9, 1, 3, 3), padding=1)        # 4 where tap t is in the frame
    want = torch.cat([inside, torch.zeros(n, N - 9, H, W)], 1)
    got = got.float().cpu().reshape(n, H, W, N).permute(0, 3, 1, 2)
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want)
        raise AssertionError(f"{name_of(case)}: {bad.shape[0]} outputs are not the exact 4 / 0 pattern; first (frame, tap, y, x): "
                             f"{bad[:8].tolist()} got {[float(got[tuple(b)]) for b in bad[:8]]}")


# ------------------------------------------------------------------------------------------------ d. impulse
@pytest.mark.parametrize("dtype", DTYPES)
@cases_of(S.IMPULSE)
def test_impulse_every_tap_chunk_edge_and_border(dtype, case):
    """One-hot weights on integer inputs: output column 4 t + j is tap t of channel c_j, c_j on both sides of the chunk edge and at
    both ends of Cin, so every output is ONE input value or 0 - the shifted, zero-padded (nearest-upsampled) input, exactly.  Whole
    frames, ragged frames with overlapped last patches in either or both directions, the x2 loader; both patch heights."""
    o = ops()
    c, g = S.full(case), S.geometry(case, dtype)
    Cin, N, H, W, n, ups = g["Cin"], c["N"], c["H"], c["W"], c["n"], c["ups"]
    He, We = S.frame(case)
    ar = torch.arange
    x = ((131 * ar(n)[:, None, None, None] + 17 * ar(Cin)[None, :, None, None] + 29 * ar(H)[None, None, :, None] + 7 * ar(W)[None, None, None, :]) % 255 - 127).float()
    chans = S.impulse_channels(dtype)
    wt = torch.zeros(N, Cin, 3, 3)
    xp = F.pad(up2(x, ups), (1, 1, 1, 1))
    want = torch.zeros(n, N, He, We)
    for t in range(9):
        for j, cj in enumerate(chans):
            wt[4 * t + j, cj, t // 3, t % 3] = 1.0
            want[:, 4 * t + j] = xp[:, cj, t // 3:t // 3 + He, t % 3:t % 3 + We]
    got, Ho, Wo = o.conv3x3(dev(to_rows(x), dtype), dev(pack_w(wt), dtype), None, n, H, W, upsample2x=ups, split_k=1, tile=S.tile_bits(case))
    assert (Ho, Wo) == (He, We)
    got = got.float().cpu().reshape(n, He, We, N).permute(0, 3, 1, 2)
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want)
        raise AssertionError(f"{name_of(case)}: {bad.shape[0]} outputs differ from the shifted input; first (frame, column, y, x): {bad[:8].tolist()}")


# ------------------------------------------------------------------------------------------------ e. 16-row patches, ragged frames
@functools.lru_cache(maxsize=None)
def ragged_operands(dtype, H, W, N, chunks, n):
    Cin = chunks * S.bk(dtype)
    x = q(seeded_randn((n, Cin, H, W), 541), dtype)
    wt, bias = q(seeded_randn((N, Cin, 3, 3), 542) / math.sqrt(9 * Cin), dtype), 0.1 * seeded_randn((N,), 543)
    res, rb = q(seeded_randn((n, N, H, W), 544), dtype), seeded_randn((n, N), 545)
    ref = out_rows(F.conv2d(x, wt, bias, padding=1) + rb[:, :, None, None] + res)
    return dev(to_rows(x), dtype), dev(pack_w(wt), dtype), bias.to(DEV), rb.to(DEV), dev(to_rows(res), dtype), ref


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", S.RAGGED16_N)
@pytest.mark.parametrize("H,W", S.RAGGED16_FRAMES)
def test_16_row_patches_and_192_column_blocks_on_ragged_frames(dtype, H, W, N):
    """16-row patches with an overlapped last patch COLUMN (He % 16 == 0, We % 16 != 0: the planner's choice below 200 tiles is 8
    rows, and the pinned-height tests of tests/test_gpu_kernels.py use whole frames), with bias, per-frame row bias and residual,
    against the f32 conv.  Widths that are odd multiples of 64 run in every launch shape - one launch (tile bit 4), 128 + 64 (bit
    8), 192-column blocks (bit 16) - and those must agree bit for bit, as they do on whole frames.  Whether 8-row patches give the
    same bits is printed, not asserted."""
    o = ops()
    case = S.ragged16_case(H, W, N)
    rows, wp, bd, rbd, rrows, ref = ragged_operands(dtype, H, W, N, case["chunks"], case["n"])
    run = lambda bits: o.conv3x3(rows, wp, bd, case["n"], H, W, rowbias=rbd, rows_per_batch=H * W, residual=rrows, split_k=1, tile=bits)[0]
    got = run(2)
    close(got, ref, dtype)
    if N in (192, 320):
        shapes = {bit: run(2 | bit) for bit in (4, 8, 16)}
        for bit, y in shapes.items():
            close(y, ref, dtype)
            assert torch.equal(y, shapes[4]), f"launch shape 2|{bit} differs from 2|4 at {H}x{W} N={N}"
        assert torch.equal(got, shapes[16])      # (few patches: the planner's own choice is the 192-column blocks)
    print(f"{H}x{W} N={N} {dtype}: 8-row patches give {'the same' if torch.equal(run(1), got) else 'other'} bits as 16-row patches")


# ------------------------------------------------------------------------------------------------ f. strides and epilogue paths
@functools.lru_cache(maxsize=None)
def epi_operands(dtype, H, W, N, chunks, n, gn):
    """operands and the f32 reference up to the row bias (no residual, no scale) of a group-f shape"""
    Cin = chunks * S.bk(dtype)
    x = q(seeded_randn((n, Cin, H, W), 551), dtype)
    wt, bias = q(seeded_randn((N, Cin, 3, 3), 552) / math.sqrt(9 * Cin), dtype), 0.1 * seeded_randn((N,), 553)
    res, rb = q(seeded_randn((n, N, H, W), 554), dtype), seeded_randn((n, N), 555)
    coef = None
    xin = x
    if gn:
        scale, shift = 1 + 0.2 * seeded_randn((n, Cin), 556), 0.3 * seeded_randn((n, Cin), 557)
        coef = coef_table(scale, shift).to(DEV)
        xin = gn_ref(x, scale, shift, torch.arange(n), True, dtype)
    y0 = out_rows(F.conv2d(xin, wt, bias, padding=1) + rb[:, :, None, None])
    return dict(x=dev(to_rows(x), dtype), w=dev(pack_w(wt), dtype), bias=bias.to(DEV), rb=rb.to(DEV), res=dev(to_rows(res), dtype),
                res_cpu=to_rows(res), y0=y0, coef=coef)


def run_epi(case, dtype, inplace_from=None):
    """launch one group-f case; returns (output view, reference).  inplace_from: the residual rows the output buffer starts from."""
    o = ops()
    c, g = S.full(case), S.geometry(case, dtype)
    Cin, N, H, W, n = g["Cin"], c["N"], c["H"], c["W"], c["n"]
    M = n * H * W
    op = epi_operands(dtype, H, W, N, c["chunks"], n, c["gn"])
    a = op["x"]
    if c["lda_pad"]:
        wide = torch.full((M, g["lda"]), 7.0, device=DEV, dtype=dtype)      # the neighbour's columns must not leak into the halo
        wide[:, :Cin] = op["x"]
        a = wide[:, :Cin]
    buf, c0 = torch.full((M + 3, g["ldc"]), SENTINEL, device=DEV, dtype=dtype), (S.C0 if c["ldc"] else 0)
    view = buf[:M, c0:c0 + N]
    y, res = op["y0"], None
    if c["residual"] == 1:
        rbuf = torch.full((M, g["ldr"]), SENTINEL, device=DEV, dtype=dtype)
        rbuf[:, :N] = op["res"]
        res = rbuf[:, :N]
    elif c["residual"] == 2:
        view.copy_(op["res"])
        res = view
    if c["residual"]:
        y = y + op["res_cpu"]
    y = y * c["out_scale"]
    kw = dict(gn=(op["coef"], 1, True)) if c["gn"] else {}
    got, _, _ = o.conv3x3(a, op["w"], op["bias"], n, H, W, rowbias=op["rb"], rows_per_batch=H * W, residual=res, out=view,
                          out_scale=c["out_scale"], split_k=1, tile=S.tile_bits(case), **kw)
    assert got.data_ptr() == view.data_ptr()
    keep = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
    keep[:M, c0:c0 + N] = False
    assert bool((buf[keep] == SENTINEL).all()), f"{name_of(case)}: wrote outside the M x N view"
    return view, y


@pytest.mark.parametrize("dtype", DTYPES)
@cases_of(S.EPI)
def test_strided_operands_and_epilogue_paths(dtype, case):
    """The input as the left part of a wider buffer (without and with the GN fold), the output as a column view of a wider buffer
    with a leading dimension that is a multiple of 8 or only of 4 (the second takes the ROW epilogue in the 2-byte types although N
    is a multiple of 8; the columns around the view keep their bits), a residual with such leading dimensions, out_scale = 0.5
    without and with a residual - on whole frames in both patch heights, plain and folded, and on a ragged frame."""
    got, ref = run_epi(case, dtype)
    close(got, ref, dtype, scale=2.0 if case["gn"] else 1.0)


@pytest.mark.parametrize("dtype", DTYPES)
@cases_of(S.INPLACE)
def test_in_place_residual_on_whole_frames_gives_the_out_of_place_bits(dtype, case):
    """out == residual on whole frames (every pixel is stored once, by the block that read its residual): the bits of the same conv
    with the residual in a buffer of its own."""
    apart, ref = run_epi(dict(case, residual=1), dtype)
    close(apart, ref, dtype, scale=2.0 if case["gn"] else 1.0)
    inplace, _ = run_epi(case, dtype)
    assert torch.equal(inplace, apart)


@pytest.mark.parametrize("dtype", DTYPES)
@cases_of(S.INPLACE_RAGGED)
def test_in_place_residual_on_a_ragged_frame_leaves_the_halo_kernel(dtype, case):
    """On a ragged frame two blocks store the overlapped pixels; in place the second would read the first one's sum as its residual.
    halo_conv_ok sends the conv to the im2col loader: both plans must say so, and the result must be the out-of-place conv."""
    o = ops()
    g = S.geometry(case, dtype)
    assert S.plan(case, dtype) == (0,) * 8 and S.plan(dict(case, residual=1), dtype)[0] == 1
    conv = dict(H=case["H"], W=case["W"], Cin=g["Cin"], stride=1, Ho=case["H"], Wo=case["W"])
    fam, _tile, _phase, flags = o.gemm_plan(dtype=dtype, M=case["n"] * case["H"] * case["W"], N=case["N"], K=9 * g["Cin"], conv=conv, bias=True,
                                            rowbias=True, rows_per_batch=case["H"] * case["W"], residual=True, split_k=1, tile=S.tile_bits(case))[:4]
    assert fam == 0 and flags & 1
    apart, ref = run_epi(dict(case, residual=1), dtype)
    close(apart, ref, dtype)
    inplace, _ = run_epi(case, dtype)
    close(inplace, ref, dtype)
    close(inplace, apart.float().cpu(), dtype)
