"""Host restatement of the frame interpolation (EMOAnimationPipeline.py:479-512 around magicanimate/utils/util.py:125-138), shared by the
GPU tests of emo_interp_frames and of `__call__(interpolation_factor=)`: the arithmetic in a chosen precision, the per-case error bound
taken from the reference arithmetic's own f32 error, and the construction of frame pairs at a given cosine."""
import torch


def slerp(v0, v1, t, thr=0.9995):
    dot = ((v0 / v0.norm()) * (v1 / v1.norm())).sum()
    if dot.abs() > thr:
        return (1.0 - t) * v0 + t * v1
    om = dot.acos()
    return (((1.0 - t) * om).sin() * v0 + (t * om).sin() * v1) / om.sin()


def linear(v0, v1, t):
    return (1.0 - t) * v0 + t * v1


def interp(lat, k, method, dtype=torch.float64, thr=0.9995):
    """lat (B, C, F, H, W) on the CPU -> (B, C, (F - 1) k + 1, H, W) computed in `dtype`; a frame is the whole lat[:, :, i] slice"""
    x = lat.to(dtype)
    B, C, F, H, W = x.shape
    out = torch.zeros(B, C, (F - 1) * k + 1, H, W, dtype=dtype)
    for j in range((F - 1) * k + 1):
        p, r = divmod(j, k)
        if r == 0:
            out[:, :, j] = x[:, :, p]
        else:
            v0, v1 = x[:, :, p], x[:, :, p + 1]
            out[:, :, j] = slerp(v0, v1, r / k, thr) if method == "slerp" else linear(v0, v1, r / k)
    return out


def generated(t, k):
    """the frames of an interpolated clip that are not copies"""
    idx = [j for j in range(t.shape[2]) if j % k]
    return t[:, :, idx]


def reference_and_bound(lat, k, method, thr=0.9995):
    """(f64 result, bound): the bound is max(4 e_ref, 2^-21 max|frame|), e_ref the largest error over the generated frames of the
    reference arithmetic run in f32 against the f64 result.  4 x: another summation order, device sin / acos a few ulp from libm.
    The floor: two roundings of a linear blend, for the cases where the f32 reference happens to be exact."""
    ref64 = interp(lat, k, method, torch.float64, thr)
    ref32 = interp(lat, k, method, torch.float32, thr)
    e_ref = float((generated(ref32, k).double() - generated(ref64, k)).abs().max())
    floor = 2.0 ** -21 * float(lat.abs().max())
    return ref64, max(4.0 * e_ref, floor), e_ref


def pair_at_cosine(n, cos, seed, scale=1.3, base=None):
    """two f32 vectors of n elements whose f64 cosine is `cos` (up to the f32 rounding of the second), |v1| = scale |v0|; the second is
    built in f64 from the first (`base`, or a seeded draw)"""
    g = torch.Generator().manual_seed(seed)
    v0 = (torch.randn(n, generator=g, dtype=torch.float64).float() if base is None else base.reshape(-1)).double()
    w = torch.randn(n, generator=g, dtype=torch.float64)
    w = w - (w @ v0) / (v0 @ v0) * v0                       # orthogonal to v0
    w = w / w.norm() * v0.norm()
    v1 = scale * (cos * v0 + (1.0 - cos * cos) ** 0.5 * w)
    return v0.float(), v1.float()


def cosine64(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a @ b) / (a.norm() * b.norm()))
