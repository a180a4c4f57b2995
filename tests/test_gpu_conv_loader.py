"""GPU parity tests of the im2col conv loader (csrc/gemm_impl.h gemm_kernel<T, CONV = true, ...>): every 3x3 conv the halo-reuse
kernel does NOT serve - stride 2, frames narrower than 16 pixels, Cin that is not a multiple of the K-tile, split-K, the VAE
encoder's asymmetric padding (conv_asym), nearest upsampling to an explicit size (up_h / up_w) - against F.conv2d in f32 on the CPU
on the same (quantised) inputs, at the tolerances of tests/test_gpu_kernels.py.  Every case is built so that gemm.hip
halo_conv_ok refuses it (`_assert_loader`); otherwise a test would silently measure the other kernel."""
import math

import pytest
import torch
import torch.nn.functional as F

from emote_hack_amd.synth import seeded_randn
from tests.test_gpu_kernels import DEV, DTYPES, close, ops, q

pytestmark = pytest.mark.gpu

TILES = [0, 1, 2, 3, 4, 7]      # planned, 64x64, 128x128, 128x160, 256x256, 7 = the ping-pong id (a conv falls back to lockstep 256x256)
VARIANTS = ["s1", "s2", "s2asym", "up2", "upto"]


def nearest_index(n_in: int, n_out: int) -> torch.Tensor:
    """Source index of every destination index of a nearest resize n_in -> n_out, the way F.interpolate(size=..., mode="nearest")
    forms it: f32 scale n_in / n_out, floor of the f32 product, clamped to n_in - 1.  (tests/test_host_logic.py holds this helper
    against F.interpolate itself on an index ramp, on any machine.)"""
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    return torch.floor(torch.arange(n_out, dtype=torch.float32) * scale).to(torch.int64).clamp(max=n_in - 1)


def bk(dtype) -> int:
    """elements of K per stage of the loader (128 bytes)"""
    return 32 if dtype == torch.float32 else 64


def _assert_loader(o, rows, wp, n, H, W, dtype, variant, split_k):
    """the case must be one gemm.hip halo_conv_ok refuses"""
    cin = wp.shape[1] // 9
    # (the halo kernel also serves the x2 upsampling, on the doubled frame; stride 2, asym and an explicit size are never its cases)
    He, We = (2 * H, 2 * W) if variant == "up2" else (H, W)
    why = variant not in ("s1", "up2") or We < 16 or He < 8 or cin % bk(dtype) != 0 or (split_k or 1) > 1 or wp.shape[0] % 4 != 0
    assert why, "this conv would run on the halo-reuse kernel"
    if variant == "s1":
        assert not o.conv_gn_fusable(rows, wp, n, H, W)


def to_rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def pack_w(wt):
    """(Cout, Cin, 3, 3) -> the re-laid (Cout, 9 * Cin) weight: tap-major, channel fastest"""
    return wt.permute(0, 2, 3, 1).reshape(wt.shape[0], -1).contiguous()


def upto_size(H, W):
    return (max(2 * H - 1, 1), max(2 * W - 1, 1))


def conv_ref(x, wt, bias, variant, size=None, device="cpu"):
    """the f32 statement of each variant, NCHW in, rows out (on the CPU; the large cases pass device=DEV, as the many-tile GEMM tests do)"""
    x, wt, bias = x.to(device), wt.to(device), bias.to(device) if bias is not None else None
    if variant == "s1":
        y = F.conv2d(x, wt, bias, padding=1)
    elif variant == "s2":
        y = F.conv2d(x, wt, bias, stride=2, padding=1)
    elif variant == "s2asym":
        y = F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, bias, stride=2, padding=0)
    elif variant == "up2":
        y = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), wt, bias, padding=1)
    else:
        y = F.conv2d(F.interpolate(x, size=tuple(size), mode="nearest"), wt, bias, padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, wt.shape[0]).cpu(), tuple(y.shape[-2:])


def conv_hip(o, rows, wp, bias, n, H, W, variant, size=None, **kw):
    a = dict(s1={}, s2=dict(stride=2), s2asym=dict(stride=2, pad=0), up2=dict(upsample2x=True), upto=dict(upsample_to=size))[variant]
    return o.conv3x3(rows, wp, bias, n, H, W, **a, **kw)


def dev(t, dtype):
    return t.to(DEV).to(dtype)


# ------------------------------------------------------------------------------------------------ 1. variant x tile matrix
# (a one-row frame has no asym case: padded (0, 1) it is lower than the 3x3 window - no output exists)
MATRIX = [(v, n, H, W) for v in VARIANTS for n, H, W in [(2, 5, 3), (1, 9, 17), (3, 1, 7), (2, 2, 2)] if not (v == "s2asym" and H < 2)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant,n,H,W", MATRIX)
def test_loader_variant_tile_matrix(dtype, variant, n, H, W):
    """Every loader variant on every tile it is instantiated for, single pass and split 3 ways over K, on odd frames (stride 2 ends
    on a half window; asym's last row / column sees the one padded line), a one-row frame and a 2x2 frame.  Cin = 24 is not a
    multiple of the K-tile in any type, so a stage straddles taps and no case is the halo kernel's; K = 216 is 4 stages in the 2-byte
    types, so the third K slice is EMPTY there.  Every tile must give the f32 conv.  Bit equality: tile 7 is not instantiated for the
    conv loader and dispatches to the very kernel of tile 4, and every launch is deterministic (the split-K partials are reduced in a
    fixed order), so those pairs are compared with torch.equal; across DIFFERENT tile shapes the single pass also gives the same bits
    (every accumulator starts from the bias and adds the same K stages in the same order, 32x32 MFMA blocks in every shape)."""
    o = ops()
    Cin, Cout = 24, 40
    x = q(seeded_randn((n, Cin, H, W), 401), dtype)
    wt, bias = q(seeded_randn((Cout, Cin, 3, 3), 402) / math.sqrt(9 * Cin), dtype), 0.1 * seeded_randn((Cout,), 403)
    size = upto_size(H, W) if variant == "upto" else None
    ref, hw = conv_ref(x, wt, bias, variant, size)
    rows, wp, bd = dev(to_rows(x), dtype), dev(pack_w(wt), dtype), bias.to(DEV)
    got = {}
    for sk in (1, 3):
        _assert_loader(o, rows, wp, n, H, W, dtype, variant, sk)
        for tile in TILES:
            y, Ho, Wo = conv_hip(o, rows, wp, bd, n, H, W, variant, size, tile=tile, split_k=sk)
            assert (Ho, Wo) == hw
            close(y, ref, dtype)
            got[sk, tile] = y
        assert torch.equal(got[sk, 7], got[sk, 4])
        again, _, _ = conv_hip(o, rows, wp, bd, n, H, W, variant, size, tile=2, split_k=sk)
        assert torch.equal(again, got[sk, 2])
    diff = [tile for tile in TILES if not torch.equal(got[1, tile], got[1, 2])]
    assert not diff, f"tiles {diff}: the single pass differs from the 128x128 tile's bits"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,Cin", [(24, 1280), (24, 2560), (10, 1280), (10, 2560)])
def test_loader_8x8_level_at_bench_widths(dtype, n, Cin):
    """The 8x8 level of the bench (M = 1536) and of the ReferenceNet group (M = 640), Cin 1280 / 2560 -> Cout 1280: every tile, single
    pass and split 4 ways, and with split_k = None, i.e. the planner's own choice - in the 2-byte types 256x256 tiles split up to 32
    ways (gemm_api.h plan_gemm `deep`).  f32 keeps n = 2 / 3 (and its reference on the CPU; the 2-byte cases take F.conv2d in f32 on
    the device).  Repeated launches are bit-identical (fixed-order reduction)."""
    o = ops()
    if dtype == torch.float32:
        n = 2 if n == 24 else 3
    H = W = 8
    Cout = 1280
    x = q(seeded_randn((n, Cin, H, W), 411), dtype)
    wt, bias = q(seeded_randn((Cout, Cin, 3, 3), 412) / math.sqrt(9 * Cin), dtype), 0.1 * seeded_randn((Cout,), 413)
    ref, _ = conv_ref(x, wt, bias, "s1", device="cpu" if dtype == torch.float32 else DEV)
    rows, wp, bd = dev(to_rows(x), dtype), dev(pack_w(wt), dtype), bias.to(DEV)
    _assert_loader(o, rows, wp, n, H, W, dtype, "s1", 1)
    if dtype != torch.float32:
        from emote_hack_amd import _lib
        sk = _lib.load().emo_gemm_suggest_split_k(n * H * W, Cout, 9 * Cin, o.dt(dtype), 0, 0)
        assert sk > 4, f"the planner was expected to split this long-K conv deeply (got {sk})"
    y0, _, _ = o.conv3x3(rows, wp, bd, n, H, W, split_k=None)
    close(y0, ref, dtype)
    y1, _, _ = o.conv3x3(rows, wp, bd, n, H, W, split_k=None)
    assert torch.equal(y0, y1)
    for sk in (1, 4):
        for tile in TILES:
            y, _, _ = o.conv3x3(rows, wp, bd, n, H, W, tile=tile, split_k=sk)
            close(y, ref, dtype)
            if tile in (0, 4):
                again, _, _ = o.conv3x3(rows, wp, bd, n, H, W, tile=tile, split_k=sk)
                assert torch.equal(y, again)


# ------------------------------------------------------------------------------------------------ 2. tap arithmetic
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", ["s1", "s2", "s2asym"])
def test_loader_tap_arithmetic_over_cin(dtype, variant):
    """Cin on both branches of `cin_aligned` (a multiple of the K-tile: the tap is wave-uniform; otherwise a K stage straddles two
    taps and the last one is ragged), on 6 x 7 frames (narrower than the halo kernel's patch)."""
    o = ops()
    n, H, W, Cout = 2, 6, 7, 40
    for Cin in ([4, 12, 36, 64] if dtype == torch.float32 else [8, 16, 24, 40, 72, 320, 328]):
        x = q(seeded_randn((n, Cin, H, W), 421), dtype)
        wt, bias = q(seeded_randn((Cout, Cin, 3, 3), 422) / math.sqrt(9 * Cin), dtype), 0.1 * seeded_randn((Cout,), 423)
        ref, hw = conv_ref(x, wt, bias, variant)
        rows, wp, bd = dev(to_rows(x), dtype), dev(pack_w(wt), dtype), bias.to(DEV)
        _assert_loader(o, rows, wp, n, H, W, dtype, variant, 1)
        for tile, sk in ((0, 1), (1, 1), (2, 1), (2, 2)):
            y, Ho, Wo = conv_hip(o, rows, wp, bd, n, H, W, variant, tile=tile, split_k=sk)
            assert (Ho, Wo) == hw
            close(y, ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Cout", [4, 6, 37])
def test_loader_narrow_and_ragged_cout(dtype, Cout):
    """Cout = 4 (conv_out) and Cout that is not a multiple of 4 (the scalar store path): single pass only - split-K needs
    N % 4 == 0 and must refuse the others, not mangle them."""
    from emote_hack_amd._lib import EmoHipError
    o = ops()
    n, H, W, Cin = 2, 8, 8, 64
    x = q(seeded_randn((n, Cin, H, W), 431), dtype)
    wt, bias = q(seeded_randn((Cout, Cin, 3, 3), 432) / math.sqrt(9 * Cin), dtype), 0.1 * seeded_randn((Cout,), 433)
    rows, wp, bd = dev(to_rows(x), dtype), dev(pack_w(wt), dtype), bias.to(DEV)
    for variant in ("s1", "s2"):
        ref, _ = conv_ref(x, wt, bias, variant)
        _assert_loader(o, rows, wp, n, H, W, dtype, variant, 1)
        for tile in (0, 1, 2, 4):
            y, _, _ = conv_hip(o, rows, wp, bd, n, H, W, variant, tile=tile, split_k=1)
            close(y, ref, dtype)
        if Cout % 4:
            with pytest.raises(EmoHipError):
                conv_hip(o, rows, wp, bd, n, H, W, variant, split_k=2)
        else:
            y, _, _ = conv_hip(o, rows, wp, bd, n, H, W, variant, split_k=2)
            close(y, ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("Cin", [16, 24, 64])
def test_loader_impulse_names_the_tap_and_channel(dtype, variant, Cin):
    """The conv loader's counterpart of the A = I check: every image holds ONE 1 - at a corner, an edge centre or an interior pixel, in
    channel 0, 5 or Cin - 1 - and the weights are small integers that differ per tap, per input channel (mod 8) and per output
    channel (mod 3): w = 1 + tap + 9 * (ci % 8) + 73 * (co % 3) <= 218, exact in bf16.  Each output is then one weight or 0 - it names
    the tap and the channel that were read - and must EQUAL the f32 conv in all three types.  Behind an upsampling one source pixel
    covers up to 2 x 2 pixels of the frame the conv sees, so an output is a sum of up to four taps' weights: there w = 1 + tap +
    9 * (ci % 6) <= 54, and every sum stays below 256, i.e. exact in bf16 as well."""
    o = ops()
    H, W, Cout = 5, 6, 12
    pix = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1), (2, 3), (1, 1)]
    chans = [0, 5, Cin - 1]
    n = len(pix) * len(chans)
    x = torch.zeros(n, Cin, H, W)
    for i, (py, px) in enumerate(pix):
        for j, c in enumerate(chans):
            x[i * len(chans) + j, c, py, px] = 1.0
    tap = torch.arange(9.0).reshape(1, 1, 3, 3)
    if variant in ("up2", "upto"):
        wt = (1 + tap + 9 * (torch.arange(Cin) % 6).reshape(1, Cin, 1, 1)).expand(Cout, Cin, 3, 3).contiguous()
    else:
        wt = 1 + tap + 9 * (torch.arange(Cin) % 8).reshape(1, Cin, 1, 1) + 73 * (torch.arange(Cout) % 3).reshape(Cout, 1, 1, 1)
    assert torch.equal(q(wt, dtype), wt)
    size = upto_size(H, W) if variant == "upto" else None
    ref, hw = conv_ref(x, wt, None, variant, size)
    assert torch.equal(q(ref, dtype), ref) and float(ref.max()) > 9
    rows, wp = dev(to_rows(x), dtype), dev(pack_w(wt), dtype)
    for tile, sk in ((0, 1), (1, 1), (4, 1), (2, 2)):
        _assert_loader(o, rows, wp, n, H, W, dtype, variant, sk)
        y, Ho, Wo = conv_hip(o, rows, wp, None, n, H, W, variant, size, tile=tile, split_k=sk)
        assert (Ho, Wo) == hw
        assert torch.equal(y.float().cpu(), ref), f"tile {tile} split {sk}: {int((y.float().cpu() != ref).sum())} outputs name another tap / channel"


# ------------------------------------------------------------------------------------------------ 3. strided input, epilogue
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant,Cin", [("s1", 64), ("s2", 64), ("s1", 40), ("s2asym", 128), ("up2", 24)])
def test_loader_strided_input_and_full_epilogue(dtype, variant, Cin):
    """lda > Cin: the input is the left part of a wider buffer whose other columns hold 7.0 (the concat buffers of the up path) - they
    must not leak into a tap.  And the resnet epilogue through the conv loader: bias + per-frame row bias + residual, times
    out_scale, stored into a strided view whose neighbouring columns must stay untouched; single pass and split-K."""
    o = ops()
    n, H, W, Cout = 3, 6, 8, 72
    x = q(seeded_randn((n, Cin, H, W), 441), dtype)
    wt, bias = q(seeded_randn((Cout, Cin, 3, 3), 442) / math.sqrt(9 * Cin), dtype), 0.1 * seeded_randn((Cout,), 443)
    y0, (Ho, Wo) = conv_ref(x, wt, bias, variant)
    res = q(seeded_randn((n * Ho * Wo, Cout), 444), dtype)
    rb = seeded_randn((n, Cout), 445)
    ref = (y0 + rb.repeat_interleave(Ho * Wo, 0) + res) * 0.5
    wide = torch.full((n * H * W, Cin + 40), 7.0, device=DEV, dtype=dtype)
    wide[:, :Cin] = dev(to_rows(x), dtype)
    rows, wp = wide[:, :Cin], dev(pack_w(wt), dtype)
    assert rows.stride(0) > Cin
    for sk in (1, 3):
        _assert_loader(o, rows, wp, n, H, W, dtype, variant, sk)
        for tile in (0, 1, 4):
            plain, _, _ = conv_hip(o, rows, wp, bias.to(DEV), n, H, W, variant, tile=tile, split_k=sk)
            close(plain, y0, dtype)
            buf = torch.full((n * Ho * Wo, Cout + 48), -3.0, device=DEV, dtype=dtype)
            out = buf[:, 16:16 + Cout]
            y, _, _ = conv_hip(o, rows, wp, bias.to(DEV), n, H, W, variant, tile=tile, split_k=sk, rowbias=rb.to(DEV), rows_per_batch=Ho * Wo,
                               residual=dev(res, dtype), out_scale=0.5, out=out)
            assert y.data_ptr() == out.data_ptr()
            close(out, ref, dtype)
            assert bool((buf[:, :16] == -3.0).all()) and bool((buf[:, 16 + Cout:] == -3.0).all())


# ------------------------------------------------------------------------------------------------ 4. many tiles per block
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,H,W,Cin,Cout,variant", [(24, 64, 64, 320, 320, "s2"), (1100, 8, 8, 64, 64, "s1")])
def test_loader_many_tiles_per_persistent_block(dtype, n, H, W, Cin, Cout, variant):
    """A persistent block walking several tiles with the conv loader (the loader's row table is rebuilt per tile while the previous
    tile's epilogue runs): the 64x64 -> 32x32 downsampler at bench size (M = 24576: 576 tiles of 128x128, 1920 of 64x64), and a stride-1
    conv on 8-pixel frames with M = 70400 (550 tiles of 128 rows, more than the 512 resident blocks).  Into a NaN-poisoned output:
    every element must have been written, and be the f32 conv (F.conv2d in f32 on the device)."""
    o = ops()
    x = q(seeded_randn((n, Cin, H, W), 451), dtype)
    wt, bias = q(seeded_randn((Cout, Cin, 3, 3), 452) / math.sqrt(9 * Cin), dtype), 0.1 * seeded_randn((Cout,), 453)
    ref, (Ho, Wo) = conv_ref(x, wt, bias, variant, device=DEV)
    rows, wp = dev(to_rows(x), dtype), dev(pack_w(wt), dtype)
    _assert_loader(o, rows, wp, n, H, W, dtype, variant, 1)
    for tile in (0, 1, 2):
        out = torch.full((n * Ho * Wo, Cout), float("nan"), device=DEV, dtype=dtype)
        conv_hip(o, rows, wp, bias.to(DEV), n, H, W, variant, tile=tile, split_k=1, out=out)
        assert bool(torch.isfinite(out).all()), f"tile {tile}: unwritten outputs"
        close(out, ref, dtype)


# ------------------------------------------------------------------------------------------------ 5. explicit-size upsampling
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,W", [(3, 5), (10, 6), (7, 7), (1, 4)])
def test_loader_upsample_to_odd_sizes(dtype, H, W):
    """unet_controlnet.py:357-365,456-459: latents that are not a multiple of 2^num_upsamplers make the upsamplers resize to the
    skip's size - (2H - 1, 2W), (2H, 2W - 1), (2H - 1, 2W - 1) - against F.interpolate(size=...) -> conv.  And up = (2H, 2W) passed
    EXPLICITLY (ops.conv3x3 would divert that size to the x2 path): the general index must reproduce the shift, bit for bit."""
    o = ops()
    n, Cin, Cout = 2, 24, 40
    x = q(seeded_randn((n, Cin, H, W), 461), dtype)
    wt, bias = q(seeded_randn((Cout, Cin, 3, 3), 462) / math.sqrt(9 * Cin), dtype), 0.1 * seeded_randn((Cout,), 463)
    rows, wp, bd = dev(to_rows(x), dtype), dev(pack_w(wt), dtype), bias.to(DEV)
    for size in ((2 * H - 1, 2 * W), (2 * H, 2 * W - 1), (2 * H - 1, 2 * W - 1)):
        ref, hw = conv_ref(x, wt, bias, "upto", size)
        for tile, sk in ((0, 1), (1, 1), (2, 2)):
            y, Ho, Wo = o.conv3x3(rows, wp, bd, n, H, W, upsample_to=size, tile=tile, split_k=sk)
            assert (Ho, Wo) == hw == size
            close(y, ref, dtype)
    x2, _, _ = o.conv3x3(rows, wp, bd, n, H, W, upsample2x=True, split_k=1)
    ex = o.gemm(rows, wp, bd, conv=dict(H=H, W=W, Cin=Cin, stride=1, upsample2x=False, Ho=2 * H, Wo=2 * W, up=(2 * H, 2 * W)), split_k=1)
    assert torch.equal(ex, x2)
    close(x2, conv_ref(x, wt, bias, "up2")[0], dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,W,up", [(14, 26, (46, 44)), (26, 21, (44, 69)), (21, 14, (69, 46))])
def test_loader_upsample_to_sizes_where_the_integer_index_differs(dtype, H, W, up):
    """F.interpolate(size=...) reads source pixel min(int(floorf(dst * (float(in) / out))), in - 1).  The loader used the integer
    dst * in / out, which differs where the f32 product rounds below an integer: 14 -> 46 at dst 23 (6, not 7), 26 -> 44 at dst 22
    (12, not 13), 21 -> 69 at dst 23 and 46 (6 and 13, not 7 and 14) - on both axes here.  (This test caught it: gemm_impl.h now
    forms the index the way torch does.)  The reference resize is written both ways - F.interpolate and `nearest_index` - and they
    must agree before the conv is compared."""
    o = ops()
    n, Cin, Cout = 1, 8, 16
    x = q(seeded_randn((n, Cin, H, W), 471), dtype)
    wt, bias = q(seeded_randn((Cout, Cin, 3, 3), 472) / math.sqrt(9 * Cin), dtype), 0.1 * seeded_randn((Cout,), 473)
    iy, ix = nearest_index(H, up[0]), nearest_index(W, up[1])
    assert not torch.equal(iy, torch.arange(up[0]) * H // up[0]) and not torch.equal(ix, torch.arange(up[1]) * W // up[1])
    xi = x[:, :, iy][:, :, :, ix]
    assert torch.equal(xi, F.interpolate(x, size=up, mode="nearest"))
    ref = F.conv2d(xi, wt, bias, padding=1).permute(0, 2, 3, 1).reshape(-1, Cout)
    rows, wp, bd = dev(to_rows(x), dtype), dev(pack_w(wt), dtype), bias.to(DEV)
    for tile, sk in ((0, 1), (2, 1), (2, 2)):
        y, Ho, Wo = o.conv3x3(rows, wp, bd, n, H, W, upsample_to=up, tile=tile, split_k=sk)
        assert (Ho, Wo) == up
        close(y, ref, dtype)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_loader_refusals_launch_nothing():
    """Geometries the loader does not serve are refused with EmoHipError before anything is launched (the poisoned output stays):
    stride 3, Ho / Wo that do not follow from the geometry, up together with upsample2x, Cin that is not a multiple of the 16-byte
    vector, and the GroupNorm fold (gn=) on a conv this loader serves."""
    from emote_hack_amd._lib import EmoHipError
    o = ops()
    dtype = torch.bfloat16
    n, H, W, Cin, Cout = 2, 8, 8, 64, 32
    rows = torch.zeros(n * H * W, Cin, device=DEV, dtype=dtype)
    wp = torch.zeros(Cout, 9 * Cin, device=DEV, dtype=dtype)
    out = torch.full((4 * n * H * W, Cout), 5.0, device=DEV, dtype=dtype)
    geo = dict(H=H, W=W, Cin=Cin, stride=1, upsample2x=False, Ho=H, Wo=W)
    o.gemm(rows, wp, None, conv=geo, out=out[:n * H * W], split_k=1)                       # the base case is served ...
    assert bool((out[:n * H * W] == 0).all()) and bool((out[n * H * W:] == 5.0).all())
    out.fill_(5.0)
    coef = torch.zeros(n, 2 * Cin, device=DEV, dtype=torch.float32)
    bad = [dict(conv=dict(geo, stride=3, Ho=3, Wo=3)),
           dict(conv=dict(geo, Ho=H - 1)), dict(conv=dict(geo, Wo=W + 1)), dict(conv=dict(geo, stride=2)),
           dict(conv=dict(geo, upsample2x=True, Ho=2 * H, Wo=2 * W, up=(2 * H, 2 * W))),
           dict(conv=dict(geo, Ho=2 * H, Wo=2 * W, up=(2 * H, 0))),
           dict(conv=geo, gn=(coef, 1, True)),                                              # 8-pixel rows: not the halo kernel's
           dict(conv=dict(geo, stride=2, Ho=H // 2, Wo=W // 2), gn=(coef, 1, True))]
    for kw in bad:
        with pytest.raises(EmoHipError):
            o.gemm(rows, wp, None, out=out[:n * kw["conv"]["Ho"] * kw["conv"]["Wo"]], split_k=1, **kw)
    # Cin = 12 is not a multiple of the 8-element vector of the 2-byte types (4-element f32 serves it: test_loader_tap_arithmetic_over_cin)
    rows12 = torch.zeros(n * H * W, 16, device=DEV, dtype=dtype)[:, :12]
    wp12 = torch.zeros(Cout, 9 * 12, device=DEV, dtype=dtype)
    with pytest.raises(EmoHipError):
        o.gemm(rows12, wp12, None, conv=dict(geo, Cin=12), out=out[:n * H * W], split_k=1)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
