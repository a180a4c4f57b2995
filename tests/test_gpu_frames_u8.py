"""GPU tests of emo_rows_to_frames_u8 (ops.rows_to_frames_u8) and AutoencoderKL.decode_video(output="uint8"): decoded NHWC rows -> packed
8-bit frames, the `/ 2 + 0.5`, `clamp(0, 1)` of decode_latents followed by save_videos_grid's `(x * 255).astype(uint8)`
(magicanimate/utils/util.py:21-33).  Every comparison is exact: with mul = 0.5 (or 1) the product inside the fused multiply-add is exact,
so the fused and the unfused form round alike and a difference of one count is a bug."""
import pytest
import torch

from emote_hack_amd.synth import seeded_randn
from tests.test_gpu_kernels import DEV, DTYPES, ops

pytestmark = pytest.mark.gpu
NAN = float("nan")
GEOMS = [(1, 3, 5), (2, 8, 8), (3, 17, 9)]        # n*H*W*3 = 45, 384 (a multiple of 16), 1377


def wide_view(t, dtype, left=8, right=8, poison=NAN):
    """t (M, C) as the columns [left, left + C) of a wider device buffer whose other columns hold `poison` (tests/test_gpu_small_ops.py)"""
    M, Cc = t.shape
    ld = (left + Cc + right + 7) // 8 * 8
    buf = torch.full((M, ld), poison, device=DEV, dtype=dtype)
    buf[:, left:left + Cc] = t.to(DEV).to(dtype)
    return buf, buf[:, left:left + Cc]


def want_u8(x, mul=0.5, add=0.5, lo=0.0, hi=1.0):
    """x (M, 3) in the compute dtype on the CPU -> the bytes torch makes of it, op by op in f32"""
    return (((x.float() * mul + add).clamp(lo, hi)) * 255).to(torch.uint8)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,H,W", GEOMS)
def test_rows_to_frames_u8_is_exact(n, H, W, dtype):
    o = ops()
    M = n * H * W
    x = (seeded_randn((M, 3), 300 + M) * 1.5).to(dtype)                          # both clamps fire
    want = want_u8(x).reshape(1, n, H, W, 3)
    assert int(want.min()) == 0 and int(want.max()) == 255 and 0 < int((want == 0).sum()) < want.numel() // 2
    rows8 = torch.zeros(M, 8, device=DEV, dtype=dtype)
    rows8[:, :3] = x.to(DEV)
    got = o.rows_to_frames_u8(rows8[:, :3], 1, 3, n, H, W)                       # contiguous ld = 8 rows (the decoder's conv_out)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, n, H, W, 3) and got.is_contiguous()
    assert torch.equal(got.cpu(), want)
    _, xv = wide_view(x, dtype)                                                  # NaN in every neighbouring column
    assert torch.equal(o.rows_to_frames_u8(xv, 1, 3, n, H, W).cpu(), want)
    assert torch.equal(o.rows_to_frames_u8(x.to(DEV).contiguous(), n, 3, 1, H, W).cpu().reshape(want.shape), want)   # ld = C, frames on the batch axis


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_to_frames_u8_other_coefficients(dtype):
    """(mul, add, lo, hi) = (1, 0, 0, 1) on multiples of 1/64 in [-0.5, 1.5): x * 255 is exact in f32"""
    o = ops()
    n, H, W = 2, 5, 7
    g = torch.Generator().manual_seed(4)
    x = ((torch.randint(0, 128, (n * H * W, 3), generator=g) - 32).float() / 64.0).to(dtype)
    want = want_u8(x, 1.0, 0.0, 0.0, 1.0).reshape(1, n, H, W, 3)
    _, xv = wide_view(x, dtype)
    assert torch.equal(o.rows_to_frames_u8(xv, 1, 3, n, H, W, 1.0, 0.0, 0.0, 1.0).cpu(), want)
    assert not torch.equal(want, want_u8(x).reshape(want.shape))


@pytest.mark.parametrize("offset", [0, 4, 1])          # the output 16-byte aligned, 4-byte aligned, unaligned
@pytest.mark.parametrize("n,H,W", GEOMS)
def test_rows_to_frames_u8_writes_nothing_past_the_end(n, H, W, offset):
    o = ops()
    M = n * H * W
    total = M * 3
    x = seeded_randn((M, 3), 310 + M) * 1.5
    buf = torch.full((offset + total + 64,), 0xA5, device=DEV, dtype=torch.uint8)
    out = buf[offset:offset + total]
    o.rows_to_frames_u8(x.to(DEV), 1, 3, n, H, W, out=out)
    assert torch.equal(out.cpu(), want_u8(x).reshape(-1))
    assert bool((buf[:offset] == 0xA5).all()) and bool((buf[offset + total:] == 0xA5).all())


def test_rows_to_frames_u8_refusals():
    from emote_hack_amd._lib import EmoHipError
    o = ops()
    x = torch.zeros(15, 8, device=DEV)
    with pytest.raises(EmoHipError):
        o.rows_to_frames_u8(x[:, :3], 1, 0, 1, 3, 5)
    with pytest.raises(EmoHipError):
        o.rows_to_frames_u8(x[:, :3].to(torch.float64), 1, 3, 1, 3, 5)


def test_decode_video_uint8_is_the_float_video_times_255():
    from tests.test_gpu_vae import SMALL, build
    m, _ = build(SMALL, torch.float32)
    lat = 0.2 * seeded_randn((1, 4, 5, 8, 8), 9)
    video = m.decode_video(lat.to(DEV), frames_per_call=2)                       # (1, 3, 5, 64, 64) f32, pinned by tests/test_gpu_vae.py
    got = m.decode_video(lat.to(DEV), frames_per_call=2, output="uint8")
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (1, 5, 64, 64, 3)
    assert torch.equal(got, (video * 255).to(torch.uint8).permute(0, 2, 3, 4, 1))
    assert len(torch.unique(got)) > 16
    two = torch.cat([lat, lat.flip(2)]).to(DEV)                                  # b = 2: frames land at (b, f)
    assert torch.equal(m.decode_video(two, frames_per_call=3, output="uint8"),
                       (m.decode_video(two, frames_per_call=3) * 255).to(torch.uint8).permute(0, 2, 3, 4, 1))
    with pytest.raises(ValueError, match="output="):
        m.decode_video(lat.to(DEV), output="int8")
