"""GPU parity tests of the small entry points either side of the loop and in the conditioning path (csrc/frontend.hip,
conditioning.hip, parts of elementwise.hip): one test per entry point, each against the torch expression include/emo_hip.h cites, at
the tolerances of tests/test_gpu_kernels.py (entry points whose output is f32 whatever the input type are held to the f32 row), at
sizes that are not multiples of the vector width or of the block, and on row views with ld > C whose neighbouring columns are
poisoned: they must be neither read into the result nor written."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from emote_hack_amd.synth import seeded_randn
from tests import cases
from tests.test_gpu_kernels import DEV, DTYPES, close, ops, q

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _lib():
    from emote_hack_amd import _lib as L
    return L.load()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def wide_view(t, dtype, left=8, right=8, poison=NAN):
    """t (M, C) as the columns [left, left + C) of a wider device buffer whose other columns hold `poison`; `left` is a multiple of
    the 16-byte vector in every type and the leading dimension is rounded up to one."""
    M, Cc = t.shape
    ld = (left + Cc + right + 7) // 8 * 8
    buf = torch.full((M, ld), poison, device=DEV, dtype=dtype)
    buf[:, left:left + Cc] = t.to(DEV).to(dtype)
    return buf, buf[:, left:left + Cc]


def untouched(buf, left, Cc, val):
    return bool((buf[:, :left] == val).all()) and bool((buf[:, left + Cc:] == val).all())


# ------------------------------------------------------------------------------------------------ frontend.hip
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 7, 63, 64, 65, 520, 4096])
def test_softmax_rows(dtype, N):
    """emo_softmax_rows against torch.softmax in f64: rows shorter than one vector per lane (idle lanes in the shuffle tree), a ragged
    tail behind the vectors, M that is not a multiple of the 4 rows of a block; scores of magnitude 1e4 at scale 1 (without the max
    subtraction exp overflows) and a row of equal values; rows sum to 1.  Input and output are column slices, starting on a 16-byte
    boundary, of wider buffers - the input's other columns hold NaN, the output's must stay as they were; N that are multiples of the
    vector also run contiguous.  A contiguous N = 7 (ld not a multiple of the vector) is refused, not mangled."""
    from emote_hack_amd._lib import EmoHipError
    o = ops()
    M = 13
    for scale, mag in ((0.125, 4.0), (1.0, 1e4)):
        x = seeded_randn((M, N), 501) * mag
        x[3] = x[3, 0]                      # a row of equal values: 1 / N each
        x = q(x, dtype)
        ref = torch.softmax(x.double() * scale, -1).float()
        assert bool(torch.isfinite(ref).all())
        xbuf, xv = wide_view(x, dtype)
        ybuf, yv = wide_view(torch.zeros(M, N), dtype, poison=-3.0)
        got = o.softmax_rows(xv, scale, out=yv)
        assert got.data_ptr() == yv.data_ptr()
        close(yv, ref, dtype)
        assert untouched(ybuf, 8, N, -3.0)
        # rows sum to 1: each stored p is rounded by at most eps / 2 of itself, so a row sum moves by at most eps / 2 from the
        # reference's; the f32 arithmetic in front of it (exponents of at most 2^5 in size, one reciprocal) adds a few 1e-6
        torch.testing.assert_close(yv.double().sum(-1).cpu(), ref.double().sum(-1), rtol=0, atol=torch.finfo(dtype).eps / 2 + 1e-5)
        close(yv[3], torch.full((N,), 1.0 / N), dtype)
        if N % 8 == 0:
            close(o.softmax_rows(x.to(DEV).to(dtype), scale), ref, dtype)
    if N == 7:
        with pytest.raises(EmoHipError):
            o.softmax_rows(x.to(DEV).to(dtype), 1.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,H,W,Cc", [(2, 5, 7, 13), (1, 2, 2, 8), (3, 9, 4, 33), (1, 16, 16, 64)])
def test_maxpool2x2(dtype, n, H, W, Cc):
    """nn.MaxPool2d(2, 2) over NHWC rows: odd H and W (floor: the last line is dropped), all-negative inputs (a zero-initialised maximum
    would show), a channel count that is not a multiple of anything - EQUAL to F.max_pool2d; input a view with ld > C whose
    neighbours hold a value that would win every maximum; and into a strided output."""
    o = ops()
    x = q(-0.5 - seeded_randn((n, Cc, H, W), 511).abs(), dtype)
    ref = F.max_pool2d(x, 2, 2).permute(0, 2, 3, 1).reshape(-1, Cc)
    _, xv = wide_view(x.permute(0, 2, 3, 1).reshape(-1, Cc), dtype, poison=1e4)
    got = o.maxpool2x2(xv, n, H, W)
    assert tuple(got.shape) == (n * (H // 2) * (W // 2), Cc)
    assert torch.equal(got.float().cpu(), ref)
    ybuf, yv = wide_view(torch.zeros_like(ref), dtype, poison=-3.0)
    rc = _lib().emo_maxpool2x2(C.c_void_p(xv.data_ptr()), xv.stride(0), C.c_void_p(yv.data_ptr()), yv.stride(0), n, H, W, Cc, o.dt(dtype), _st())
    assert rc == 0 and torch.equal(yv.float().cpu(), ref) and untouched(ybuf, 8, Cc, -3.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,w,Ho,Wo", [(7, 5, 64, 64), (64, 64, 9, 11), (16, 16, 16, 16), (3, 1, 5, 4)])
def test_bilinear_to_nchw(dtype, h, w, Ho, Wo):
    """F.interpolate(size=..., mode="bilinear", align_corners=False) of NHWC rows into NCHW f32: up- and down-scaling at non-integer
    ratios, a one-column source, and the identity, which is exact.  f32 output from exact inputs: the f32 row of TOL in every type."""
    o = ops()
    n, Cc = 2, 5
    x = q(seeded_randn((n, Cc, h, w), 521), dtype)
    ref = F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=False)
    _, xv = wide_view(x.permute(0, 2, 3, 1).reshape(-1, Cc), dtype)
    got = o.bilinear_to_nchw(xv, n, Cc, h, w, Ho, Wo)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, Cc, Ho, Wo)
    close(got, ref, torch.float32)
    if (h, w) == (Ho, Wo):
        assert torch.equal(got.cpu(), x)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mul,add,lo,hi", [(0.5, 0.5, 0.0, 1.0), (0.7, -0.2, -0.5, 0.9)])
def test_rows_to_video(dtype, mul, add, lo, hi):
    """decode_latents' `(video / 2 + 0.5).clamp(0, 1)` and a non-default affine / clamp: rows ((b f) h w, ld > C) -> (B, C, F, H, W) f32
    with values on both sides of both bounds."""
    o = ops()
    B, Cc, Fr, H, W = 2, 3, 5, 3, 7
    x = q(seeded_randn((B * Fr * H * W, Cc), 531) * 1.5, dtype)
    pre = x * mul + add
    assert bool((pre < lo).any()) and bool((pre > hi).any()) and bool(((pre > lo) & (pre < hi)).any())
    ref = pre.clamp(lo, hi).reshape(B, Fr, H, W, Cc).permute(0, 4, 1, 2, 3).contiguous()
    _, xv = wide_view(x, dtype)
    got = o.rows_to_video(xv, B, Cc, Fr, H, W, mul, add, lo, hi)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, Cc, Fr, H, W)
    close(got, ref, torch.float32)
    assert float(got.min()) == float(torch.tensor(lo, dtype=torch.float32)) and float(got.max()) == float(torch.tensor(hi, dtype=torch.float32))
    if (mul, add, lo, hi) == (0.5, 0.5, 0.0, 1.0):
        close(o.rows_to_video(xv, B, Cc, Fr, H, W), ref, torch.float32)      # the defaults are decode_latents'


# ------------------------------------------------------------------------------------------------ conditioning.hip
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,Cc,rpb", [(37, 13, 10), (64, 320, 64), (5, 8, 1)])
def test_add_rowbias(dtype, M, Cc, rpb):
    """y[m] = x[m] + rb[m // rows_per_batch] with a ragged last batch; x, rb and y are views with ld > C (poisoned neighbours)."""
    o = ops()
    nb = (M + rpb - 1) // rpb
    x, rb = q(seeded_randn((M, Cc), 541), dtype), q(seeded_randn((nb, Cc), 542), dtype)
    ref = x + rb[torch.arange(M) // rpb]
    _, xv = wide_view(x, dtype)
    _, rv = wide_view(rb, dtype)
    close(o.add_rowbias(xv, rv, rpb), ref, dtype)
    ybuf, yv = wide_view(torch.zeros(M, Cc), dtype, poison=-3.0)
    rc = _lib().emo_add_rowbias(C.c_void_p(xv.data_ptr()), xv.stride(0), C.c_void_p(rv.data_ptr()), rv.stride(0), C.c_void_p(yv.data_ptr()), yv.stride(0),
                                M, Cc, rpb, o.dt(dtype), _st())
    assert rc == 0
    close(yv, ref, dtype)
    assert untouched(ybuf, 8, Cc, -3.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_rows(dtype):
    """nn.Embedding lookup: first and last row, repeated indices, a width that is not a multiple of the vector - exact."""
    o = ops()
    rows, D = 9, 13
    table = q(seeded_randn((rows, D), 551), dtype)
    idx = torch.tensor([0, rows - 1, 3, 3, 0, rows - 1, 7, 3, 1], dtype=torch.int32)
    got = o.gather_rows(table.to(DEV).to(dtype), idx.to(DEV))
    assert torch.equal(got.float().cpu(), table[idx.long()])


@pytest.mark.parametrize("dtype", DTYPES)
def test_copy_cols_and_add_on_strided_views(dtype):
    """emo_copy_cols / emo_add with strided source AND destination (the concat buffers): exact copy at a column offset, a + alpha * b into
    a view; the poisoned columns either side are neither read nor written."""
    o = ops()
    M, Cc = 37, 24
    a, b = q(seeded_randn((M, Cc), 561), dtype), q(seeded_randn((M, Cc), 562), dtype)
    _, av = wide_view(a, dtype)
    _, bv = wide_view(b, dtype, left=16, right=24)
    ybuf = torch.full((M, 8 + Cc + 16 + 8), -3.0, device=DEV, dtype=dtype)
    o.copy_cols(av, ybuf[:, 8:], 16)           # columns [24, 24 + C) of the buffer
    assert torch.equal(ybuf[:, 24:24 + Cc].float().cpu(), a) and untouched(ybuf, 24, Cc, -3.0)
    sbuf, sv = wide_view(torch.zeros(M, Cc), dtype, poison=-3.0)
    got = o.add(av, bv, alpha=-0.75, out=sv)
    assert got.data_ptr() == sv.data_ptr()
    close(sv, a - 0.75 * b, dtype)
    assert untouched(sbuf, 8, Cc, -3.0)


def test_speed_encode_and_bucket():
    """SpeedEncoder.encode_speed (tanh((v - c) / r * 3), f64 reference) and SpeedController.map_speed_to_bucket (argmin |v - c|, the FIRST
    minimum on ties, INT exact against torch.argmin) over cases.SPEEDS plus values exactly half-way between two centres of each table."""
    from emote_hack_amd.conditioning import SpeedEncoder
    o = ops()
    for k, centers in enumerate((torch.linspace(-1.0, 1.0, 9), torch.tensor(SpeedEncoder.CENTERS), torch.linspace(-1.0, 1.0, 16))):
        mid = (centers[:-1] + centers[1:]) / 2
        v = torch.cat([torch.tensor(cases.SPEEDS), mid, centers])
        d = (v[:, None] - centers[None, :]).abs()
        if k == 0:      # centres on multiples of 0.25: the half-way values are exact ties in f32
            assert int(((d == d.min(1, keepdim=True).values).sum(1) >= 2).sum()) >= 8
        idx = o.speed_bucket(v.to(DEV), centers.to(DEV))
        assert idx.dtype == torch.int32 and torch.equal(idx.cpu().long(), torch.argmin(d, dim=1))
        radii = torch.full_like(centers, 0.1)
        ref = torch.tanh((v.double()[:, None] - centers.double()[None, :]) / radii.double()[None, :] * 3.0).float()
        for dtype in DTYPES:
            close(o.speed_encode(v.to(DEV), centers.to(DEV), radii.to(DEV), dtype), ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["silu", "relu", "tanh", "gelu", "quick_gelu"])
def test_act_every_kind(dtype, kind):
    """emo_act, all five kinds, on a grid through [-20, 20] plus +-100 and +-0 (1003 elements: not a multiple of the block), against
    f64 torch on the quantised inputs."""
    o = ops()
    x = q(torch.cat([torch.linspace(-20, 20, 999), torch.tensor([100.0, -100.0, 0.0, -0.0])]), dtype)
    xd = x.double()
    ref = dict(silu=F.silu, relu=F.relu, tanh=torch.tanh, gelu=F.gelu, quick_gelu=lambda t: t * torch.sigmoid(1.702 * t))[kind](xd).float()
    got = o.act(x.to(DEV).to(dtype), kind)
    assert bool(torch.isfinite(got).all())
    close(got, ref, dtype)


# ------------------------------------------------------------------------------------------------ elementwise.hip
def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16])
def test_convert_is_torch_cast_bit_for_bit(half):
    """emo_convert f32 -> f16 / bf16 and back, BIT-exact against torch's casts (round to nearest even): subnormals of the target and
    values below its smallest one, the largest finite value, values that round to infinity and the last that do not, ties that go
    to the even neighbour both ways, +-0, +-inf, and random values; widening is exact on every finite 16-bit pattern."""
    o = ops()
    fi = torch.finfo(half)
    mant = 10 if half == torch.float16 else 7
    ulp1 = 2.0 ** -mant                                   # spacing at 1.0
    tiny_sub = fi.smallest_normal * ulp1                  # the smallest subnormal
    sp = [0.0, -0.0, float("inf"), -float("inf"), 1.0, -1.0, fi.max, -fi.max, fi.smallest_normal, -fi.smallest_normal,
          tiny_sub, 3 * tiny_sub, -5 * tiny_sub, 0.5 * tiny_sub, 0.5 * tiny_sub * (1 + 2.0 ** -10), 0.25 * tiny_sub, 1.5 * tiny_sub, 2.5 * tiny_sub,
          fi.smallest_normal * (1 - ulp1), fi.smallest_normal * (1 - ulp1 / 2),
          1 + ulp1 / 2, 1 + 3 * ulp1 / 2, 1 + ulp1 / 2 + 2.0 ** -23, 1 + ulp1 / 2 - 2.0 ** -23, -(1 + ulp1 / 2), -(1 + 3 * ulp1 / 2),
          2 - ulp1 / 2, 1024 + 512 * ulp1, 1024 + 1536 * ulp1]
    top = torch.tensor(fi.max, dtype=torch.float64)
    half_ulp_top = top * (2.0 ** -(mant + 1)) / (2 - ulp1)     # half the spacing below the largest finite value
    over = [float(top + half_ulp_top), float(top + half_ulp_top * (1 - 2.0 ** -12)), float(top + 2 * half_ulp_top)]
    over = [v for v in over if v <= torch.finfo(torch.float32).max] + [torch.finfo(torch.float32).max]
    src = torch.cat([torch.tensor(sp + over + [-v for v in over], dtype=torch.float64).float(), seeded_randn((4096,), 571) * 3,
                     seeded_randn((1024,), 572) * 1e-6 * (1.0 if half == torch.float16 else 1e-33)])
    want = src.to(half)
    assert bool(torch.isinf(want[torch.isfinite(src)]).any()) and bool(((want != 0) & (want.float().abs() < fi.smallest_normal)).any())
    got = o.convert(src.to(DEV), half)
    assert got.dtype == half and torch.equal(_bits(got.cpu()), _bits(want))
    # widening: every finite 16-bit pattern
    pat = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(half)
    pat = pat[torch.isfinite(pat)]
    up = o.convert(pat.to(DEV), torch.float32)
    assert up.dtype == torch.float32 and torch.equal(_bits(up.cpu()), _bits(pat.float()))
    # ... and the round trip through f32 is the identity
    assert torch.equal(_bits(o.convert(up, half).cpu()), _bits(pat))


@pytest.mark.parametrize("dtype", DTYPES)
def test_accumulate_window(dtype):
    """noise_pred[branch, :, frames[j]] += pred rows; counter[frames[j]] += 1: pred in every type as a view with ld > C, a frame list with
    negative (skipped) positions, add_counter on and off, two calls in sequence into the same accumulator.  f32 output from exact
    inputs: the f32 row of TOL."""
    o = ops()
    C4, Ft, HW = 4, 7, 21
    frames1, frames2 = [4, -1, 0, 6], [6, 1, -2, 4]
    p1, p2 = q(seeded_randn((4 * HW, C4), 581), dtype), q(seeded_randn((4 * HW, C4), 582), dtype)
    start = seeded_randn((C4, Ft, HW), 583)
    ref, cnt_ref = start.clone(), torch.tensor([1.0, 0, 2, 0, 0, 3, 0])
    acc, cnt = start.clone().to(DEV), cnt_ref.clone().to(DEV)
    for pred, frames, add_counter in ((p1, frames1, True), (p2, frames2, False), (p2, frames2, True)):
        for j, f in enumerate(frames):
            if f >= 0:
                ref[:, f] += pred[j * HW:(j + 1) * HW].t()
                if add_counter:
                    cnt_ref[f] += 1
        _, pv = wide_view(pred, dtype)
        o.accumulate_window(pv, acc, cnt, torch.tensor(frames, dtype=torch.int32, device=DEV), C_=C4, F=Ft, HW=HW, add_counter=add_counter)
    close(acc, ref, torch.float32)
    assert torch.equal(cnt.cpu(), cnt_ref)
    untouched_frames = [2, 3, 5]
    assert torch.equal(acc[:, untouched_frames].cpu(), start[:, untouched_frames])
