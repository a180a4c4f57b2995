"""The unrolled main loop of the halo-reuse 3x3 conv (csrc/conv_halo_impl.h UNR: the nine taps of a chunk unrolled - the default on 16-row
patches of the 2-byte types, 128- and 64-column blocks) against the rolled loop it replaces, which emo_gemm_params.tile bit 5 (32)
keeps selectable (csrc/gemm.hip plan_halo).

Both loops issue the same requests, waits, barriers and MFMAs per accumulator in the same order (chunk, tap, k-step), so their outputs
must be the same BITS: a tap whose unrolled constants (halo offset, swizzle key, weight slot, halo piece) are off, a loader stream or
ring phase lost at a chunk or tile boundary shows as a difference.  The shapes are the smallest at which the schedule changes:
  * Cin 64 / 128 / 192 / 320 = 1 / 2 / 3 / 5 chunks: a one-chunk stream is prologue + drain alone (9 stages), odd and even chunk
    counts flip the halo buffer and the weight slot at a tile boundary both ways;
  * N 64 / 128 / 192 / 320: the 64-, 128- and 192-column blocks (the last keeps the rolled loop: the pair pins that), and the
    128 + 192 and (tile bit 3) 128 + 128 + 64 launch chains;
  * frames of 16 x 16 and 32 x 16, with fewer tiles than blocks (every block: prologue + drain) and with exactly 256 patches;
  * 600 frames: blocks that walk 2 to 3 tiles (the epilogue between two tiles);
  * a frame with an overlapped last patch column, the x2 upsampling, and bias + temb row bias + residual.
(A 24 x 24 frame is not a whole number of 16-row patches: it runs on 8-row patches, which keep the rolled loop - the pair is the same
launch twice and pins that bit 5 means nothing else there; 32 x 24 is the overlapped frame that does reach the unrolled loop.)

Bit identity alone would let the pair be wrong together: one case per block width is held against F.conv2d in f64 on the same rounded
operands, at the accumulation budget tests/test_gpu_precision.py derives for K = 9 Cin (tests/precision_ref.py accum_budget)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_precision import DEV, HALVES, IDS, ops

pytestmark = pytest.mark.gpu

ROLLED = 32         # emo_gemm_params.tile bit 5: the rolled main loop
PH16 = 2            # (tile & 3) == 2: 16-row patches pinned
REM64 = 8           # tile bit 3: the 64-column remainder launch instead of 192-column blocks
CINS = [64, 128, 192, 320]
WIDTHS = [64, 128, 192, 320]
FRAMES = [(16, 16), (32, 16)]


def operands(dtype, n, H, W, Cin, N, seed, He=None, We=None, epilogue=False):
    """random operands made on the device (the comparison is between two runs on the same operands)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    He, We = He or H, We or W
    x = torch.randn(n * H * W, Cin, device=DEV, generator=g).to(dtype)
    w = (torch.randn(N, 9 * Cin, device=DEV, generator=g) / math.sqrt(9 * Cin)).to(dtype)
    bias = 0.1 * torch.randn(N, device=DEV, generator=g)
    kw = {}
    if epilogue:
        kw = dict(rowbias=torch.randn(n, N, device=DEV, generator=g), rows_per_batch=He * We,
                  residual=torch.randn(n * He * We, N, device=DEV, generator=g).to(dtype))
    return x, w, bias, kw


def pair(dtype, n, H, W, Cin, N, tile=PH16, upsample2x=False, epilogue=False, seed=7001):
    """the conv on the default (unrolled) loop and on the rolled one: (unrolled, rolled)"""
    o = ops()
    He, We = (2 * H, 2 * W) if upsample2x else (H, W)
    x, w, bias, kw = operands(dtype, n, H, W, Cin, N, seed + Cin + 3 * N, He, We, epilogue)
    unrolled, _, _ = o.conv3x3(x, w, bias, n, H, W, upsample2x=upsample2x, split_k=1, tile=tile, **kw)
    rolled, _, _ = o.conv3x3(x, w, bias, n, H, W, upsample2x=upsample2x, split_k=1, tile=tile | ROLLED, **kw)
    return unrolled, rolled


def assert_same_bits(unrolled, rolled, what):
    if torch.equal(unrolled, rolled):
        return
    bad = unrolled != rolled
    rows, cols = torch.nonzero(bad.any(1)).flatten(), torch.nonzero(bad.any(0)).flatten()
    worst = float((unrolled.float() - rolled.float()).abs().max())
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outputs differ between the unrolled and the rolled loop (rows "
                         f"{rows[:6].tolist()}.. of {unrolled.shape[0]}, columns {cols[:6].tolist()}..{cols[-1:].tolist()}; max |diff| {worst:.3e})")


def plan(dtype, n, H, W, Cin, N, tile, **kw):
    """(patch height, [(block width, tiles, grid) of every launch]) of the library's own plan; the conv must be the halo kernel's"""
    served, ph, *l = ops().conv_halo_plan(dtype=dtype, n_img=n, H=H, W=W, Cin=Cin, N=N, bias=True, tile=tile, **kw)
    assert served == 1
    return ph, [tuple(l[i:i + 3]) for i in (0, 3) if l[i]]


def chains(N):
    """tile hints of the launch chains of a width: N = 192 as one 192-column launch or 128 + 64, N = 320 as 128 + 192 or 128 + 128 + 64"""
    return [PH16, PH16 | REM64] if N in (192, 320) else [PH16]


@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
@pytest.mark.parametrize("N", WIDTHS)
@pytest.mark.parametrize("Cin", CINS)
def test_unrolled_loop_gives_the_bits_of_the_rolled_loop(dtype, Cin, N):
    for H, W in FRAMES:
        per_frame = (H // 16) * (W // 16)
        for n in (3, 256 // per_frame):                    # fewer tiles than blocks / exactly 256 patches
            for tile in chains(N):
                ph, launches = plan(dtype, n, H, W, Cin, N, tile)
                want = {(64, PH16): [64], (128, PH16): [128], (192, PH16): [192], (192, PH16 | REM64): [128, 64],
                        (320, PH16): [128, 192], (320, PH16 | REM64): [128, 64]}[(N, tile)]
                assert ph == 16 and [l[0] for l in launches] == want, (N, tile, ph, launches)
                patches = n * per_frame
                for bn, tiles, grid in launches:           # (the 128-column launch of 128 + 128 + 64 has two column tiles per patch)
                    assert tiles == patches * (2 if (N, tile, bn) == (320, PH16 | REM64, 128) else 1) and grid == min(tiles, 256), launches
                unrolled, rolled = pair(dtype, n, H, W, Cin, N, tile)
                assert_same_bits(unrolled, rolled, f"{IDS(dtype)} Cin={Cin} N={N} {n}x{H}x{W} tile={tile}")


@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
@pytest.mark.parametrize("Cin,N", [(64, 128), (128, 192), (320, 64)])
def test_unrolled_loop_over_blocks_that_walk_tiles(dtype, Cin, N):
    """600 tiles on 256 blocks: blocks walk 2 to 3 tiles, at every block width"""
    n = 600
    assert plan(dtype, n, 16, 16, Cin, N, PH16) == (16, [(N, 600, 256)])
    unrolled, rolled = pair(dtype, n, 16, 16, Cin, N)
    assert_same_bits(unrolled, rolled, f"{IDS(dtype)} Cin={Cin} N={N} 600x16x16")


@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
@pytest.mark.parametrize("H,W,ph", [(24, 24, 8), (32, 24, 16)])
def test_unrolled_loop_on_overlapped_last_patches(dtype, H, W, ph):
    n, Cin, N = 5, 128, 320
    assert plan(dtype, n, H, W, Cin, N, PH16)[0] == ph
    unrolled, rolled = pair(dtype, n, H, W, Cin, N)
    assert_same_bits(unrolled, rolled, f"{IDS(dtype)} {n}x{H}x{W}")


@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
def test_unrolled_loop_under_the_x2_upsampling(dtype):
    n, H, W, Cin, N = 5, 16, 8, 192, 128
    assert plan(dtype, n, H, W, Cin, N, PH16, upsample2x=True) == (16, [(128, 10, 10)])
    unrolled, rolled = pair(dtype, n, H, W, Cin, N, upsample2x=True)
    assert_same_bits(unrolled, rolled, f"{IDS(dtype)} {n}x{H}x{W} up")


@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
def test_unrolled_loop_with_bias_row_bias_and_residual(dtype):
    n, H, W, Cin, N = 300, 16, 16, 128, 320                # 128 + 128 + 64 columns: blocks of the main launch walk 2 to 3 tiles
    assert plan(dtype, n, H, W, Cin, N, PH16, rowbias=True, rows_per_batch=H * W, residual=True) == (16, [(128, 600, 256), (64, 300, 256)])
    unrolled, rolled = pair(dtype, n, H, W, Cin, N, epilogue=True)
    assert_same_bits(unrolled, rolled, f"{IDS(dtype)} {n}x{H}x{W} bias + row bias + residual")


# one case per block width against the f64 conv of the same rounded operands: (Cin, N, tile) -> the 64-, 128- and 192-column blocks
REFERENCE = [(192, 64, PH16), (320, 128, PH16), (128, 192, PH16)]


@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
@pytest.mark.parametrize("Cin,N,tile", REFERENCE)
def test_unrolled_loop_against_the_reference_conv(dtype, Cin, N, tile):
    """|got - r| within accum_budget(K = 9 Cin + bias) of the f64 conv r on the operands as rounded to the compute dtype, and the
    misrounded share under the cap of tests/test_gpu_precision.py - on the default loop."""
    from tests.test_gpu_precision import check_accum
    o = ops()
    n, H, W = 3, 32, 16
    assert plan(dtype, n, H, W, Cin, N, tile) == (16, [(N, 6, 6)])
    x, w, bias, _ = operands(dtype, n, H, W, Cin, N, 7100 + Cin + N)
    xf = x.float().cpu().reshape(n, H, W, Cin).permute(0, 3, 1, 2)
    wf = w.float().cpu().reshape(N, 3, 3, Cin).permute(0, 3, 1, 2)
    bf = bias.cpu()
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, N)
    r = rows(F.conv2d(xf.double(), wf.double(), bf.double(), padding=1))
    sabs = rows(F.conv2d(xf.abs(), wf.abs(), bf.abs(), padding=1)).double() * (1 + 1e-5)
    case = type("Case", (), dict(r=r, sabs=sabs, terms=9 * Cin + 4))
    got, _, _ = o.conv3x3(x, w, bias, n, H, W, split_k=1, tile=tile)
    check_accum(f"conv unrolled loop {IDS(dtype)} {Cin}->{N}", got.float().cpu(), case, dtype)
