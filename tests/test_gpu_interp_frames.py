"""GPU tests of emo_interp_frames (ops.interpolate_frames, EMOAnimationPipeline.interpolate_latents on device tensors): the clip-level
frame interpolation of EMOAnimationPipeline.py:479-512 with the slerp / linear of magicanimate/utils/util.py:125-138.

The tolerance is taken per case from the reference arithmetic itself (tests/interp_ref.py reference_and_bound): with e_ref the error of
the reference arithmetic run in f32 on the CPU against its f64 restatement, the kernel's error against the same f64 result must be at
most max(4 e_ref, 2^-21 max|frame|).  Near-antiparallel slerps are ill-conditioned (sin(omega) -> 0), which is why no single constant
would do.

Observed on an MI355X (errors relative to max|frame|; the full table is in profiles/interp_frames.md):
  shape sweep, slerp:     kernel 3.8e-08 .. 8.2e-08   (e_ref 5.2e-08 .. 1.4e-07, bound 4.8e-07 .. 5.8e-07)
  shape sweep, linear:    kernel 1.5e-08 .. 6.8e-08   (e_ref the same to three digits, bound 4.8e-07 = the floor)
  cos 0, -0.5, 0.9, 0.999, +-0.9999:  kernel 1.8e-10 .. 8.1e-08   (bound 4.8e-07 .. 5.1e-07)
  cos -0.99:              kernel 3.5e-06 .. 3.9e-06   (e_ref 1.6e-05 .. 1.8e-05, bound 6.3e-05 .. 7.3e-05)
  cos -0.999:             kernel 1.2e-05 .. 1.4e-05   (e_ref 4.0e-04 .. 4.7e-04, bound 1.6e-03 .. 1.9e-03)
  reference golden:       |kernel - golden| 2.4e-07 slerp, 1.2e-07 linear (absolute; bound 1.5e-06)
"""
import os

import pytest
import torch

from emote_hack_amd.synth import seeded_randn
from tests import cases
from tests import interp_ref as R
from tests.test_gpu_kernels import DEV, ops

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 2, 3, 5),      # one pair, 60 elements, HW odd (scalar path)
          (1, 4, 3, 8, 8),      # exactly 256 per frame: one full block pass
          (1, 4, 3, 1, 257),    # HW odd and larger than a block pass
          (2, 4, 4, 5, 7),      # the batch is inside the norm
          (1, 4, 5, 33, 33)]    # 4356 per frame: several slices per pair, so the partials are combined
COSINES = [0.0, -0.5, 0.9, 0.9990, 0.9999, -0.9999, -0.9990, -0.99]


def _err(got, ref64, k):
    return float((R.generated(got.cpu().double(), k) - R.generated(ref64, k)).abs().max())


def _check(lat, k, method, what):
    ref64, bound, e_ref = R.reference_and_bound(lat, k, method)
    got = ops().interpolate_frames(lat.to(DEV), k, method)
    B, C, F, H, W = lat.shape
    assert tuple(got.shape) == (B, C, (F - 1) * k + 1, H, W) and got.dtype == torch.float32
    assert torch.equal(got[:, :, ::k].cpu(), lat), "frames j % k == 0 are copies"
    err, top = _err(got, ref64, k), float(lat.abs().max())
    print(f"interp {what} k={k} {method}: kernel err {err / top:.3e}  e_ref {e_ref / top:.3e}  bound {bound / top:.3e}  (relative to max|frame|)")
    assert err <= bound, (what, k, method, err, e_ref, bound)
    return got


@pytest.mark.parametrize("method", ["slerp", "linear"])
@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_interpolate_frames_vs_f64_restatement(shape, k, method):
    _check(seeded_randn(shape, 900 + sum(shape)), k, method, "x".join(map(str, shape)))


def _cosine_clip(cos, seed, hw=(8, 9)):
    """three frames (1, 4, 3, h, w): frame 1 at cosine `cos` to frame 0 and 1.3 times as long, frame 2 the same to frame 1"""
    n = 4 * hw[0] * hw[1]
    v0, v1 = R.pair_at_cosine(n, cos, seed)
    _, v2 = R.pair_at_cosine(n, cos, seed + 1, base=v1)
    return torch.stack([v.reshape(1, 4, *hw) for v in (v0, v1, v2)], dim=2)


@pytest.mark.parametrize("cos", COSINES)
def test_interpolate_frames_branch_cases(cos):
    """both sides of the threshold on both signs, and the ill-conditioned near-antiparallel slerps"""
    lat = _cosine_clip(cos, 40 + COSINES.index(cos))
    for i in range(2):
        c = R.cosine64(lat[:, :, i], lat[:, :, i + 1])
        assert abs(c - cos) < 1e-5 and not 0.9993 <= abs(c) <= 0.9997, (cos, c)   # never on the f32 rounding's side of the threshold
        assert abs(float(lat[:, :, i + 1].double().norm() / lat[:, :, i].double().norm()) - 1.3) < 1e-5
    for k in (2, 3):
        got = _check(lat, k, "slerp", f"cos={cos}")
        lin = R.interp(lat, k, "linear")
        is_linear = float((R.generated(got.cpu().double(), k) - R.generated(lin, k)).abs().max()) <= 2.0 ** -21 * float(lat.abs().max())
        assert is_linear == (abs(cos) > 0.9995), (cos, k)            # the device took the branch the threshold names


def test_interpolate_latents_on_the_device_is_the_reference_golden():
    """the reference's own interpolate_latents output (tests/golden/pipeline_methods.safetensors, as tests/test_host_logic.py reads it)
    through the pipeline method on device tensors"""
    from safetensors.torch import load_file
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd import pipeline as P
    g = load_file(os.path.join(cases.GOLDEN_DIR, "pipeline_methods.safetensors"))
    pipe = P.EMOAnimationPipeline(unet=type("U", (), {"device": torch.device(DEV)})(), scheduler=DDIMScheduler())
    l3 = seeded_randn((1, 4, 3, 4, 4), 502)
    before = P.get_tensor_interpolation_method()
    try:
        for name, is_slerp in (("slerp", True), ("linear", False)):
            P.set_tensor_interpolation_method(is_slerp)
            _, bound, e_ref = R.reference_and_bound(l3, 3, name)
            got = pipe.interpolate_latents(l3.to(DEV), 3, DEV)
            assert got.is_cuda and tuple(got.shape) == (1, 4, 7, 4, 4)
            err = float((got.cpu() - g[f"interpolate/{name}"]).abs().max())
            print(f"interp golden {name}: |kernel - golden| {err:.3e}  e_ref {e_ref:.3e}  bound {bound:.3e}")
            assert err <= bound
            # bf16 latents convert to f32 and back
            gb = pipe.interpolate_latents(l3.to(DEV).bfloat16(), 3, DEV)
            assert gb.dtype == torch.bfloat16
            torch.testing.assert_close(gb.float().cpu(), R.interp(l3.bfloat16().float(), 3, name).float(), rtol=2 ** -7, atol=2 ** -7)
        assert pipe.interpolate_latents(l3.to(DEV), 1, DEV).is_cuda            # factor 1: the input itself
    finally:
        P.tensor_interpolation = before


def test_identical_consecutive_frames_take_the_linear_branch():
    lat = seeded_randn((1, 4, 4, 6, 6), 77)
    lat[:, :, 2] = lat[:, :, 1]
    k = 3
    got = ops().interpolate_frames(lat.to(DEV), k, "slerp").cpu()
    assert bool(torch.isfinite(got).all())
    floor = 2.0 ** -21 * float(lat.abs().max())
    for j in (k + 1, k + 2):                                   # between input frames 1 and 2
        assert float((got[:, :, j] - lat[:, :, 1]).abs().max()) <= floor
    _check(lat, k, "slerp", "identical pair")


def test_a_zero_frame_makes_nan_only_between_it_and_its_neighbours():
    lat = seeded_randn((1, 4, 5, 8, 8), 78)
    lat[:, :, 2] = 0.0
    k = 3
    got = ops().interpolate_frames(lat.to(DEV), k, "slerp").cpu()
    nan_frames = [4, 5, 7, 8]                                   # strictly between input frame 2 (output 6) and frames 1, 3 (outputs 3, 9)
    for j in range(got.shape[2]):
        if j in nan_frames:
            assert bool(torch.isnan(got[:, :, j]).all()), j
        else:
            assert bool(torch.isfinite(got[:, :, j]).all()), j
    assert torch.equal(got[:, :, ::k], lat)
    ref64, ref32 = R.interp(lat, k, "slerp", torch.float64), R.interp(lat, k, "slerp", torch.float32)
    fine = [1, 2, 10, 11]
    e_ref = float((ref32[:, :, fine].double() - ref64[:, :, fine]).abs().max())
    bound = max(4.0 * e_ref, 2.0 ** -21 * float(lat.abs().max()))
    assert float((got[:, :, fine].double() - ref64[:, :, fine]).abs().max()) <= bound
    # linear has no norm in it: zeros blend like any frame
    assert bool(torch.isfinite(ops().interpolate_frames(lat.to(DEV), k, "linear")).all())


def test_interpolate_frames_is_deterministic():
    x = seeded_randn((1, 4, 5, 33, 33), 79).to(DEV)
    a, b = ops().interpolate_frames(x, 3, "slerp"), ops().interpolate_frames(x, 3, "slerp")
    assert torch.equal(a, b)


def test_interpolate_frames_is_capturable():
    """a host read of the dot product (the reference's `if dot.abs() > DOT_THRESHOLD`) would fail the capture"""
    o = ops()
    shape = (1, 4, 5, 33, 33)
    a, b = seeded_randn(shape, 80).to(DEV), seeded_randn(shape, 81).to(DEV)
    b[:, :, 3] = b[:, :, 2]                                     # a linear-branch pair that the captured clip does not have
    want = o.interpolate_frames(b, 3, "slerp")
    x = a.clone()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        o.interpolate_frames(x, 3, "slerp")
        with torch.cuda.graph(g, stream=s):
            y = o.interpolate_frames(x, 3, "slerp")
    torch.cuda.synchronize()
    x.copy_(b)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, want)


def test_interpolate_frames_refusals():
    from emote_hack_amd._lib import EmoHipError
    o = ops()
    x = seeded_randn((1, 4, 3, 4, 4), 82).to(DEV)
    with pytest.raises(EmoHipError):
        o.interpolate_frames(x[:, :, :1], 2)                    # F = 1
    with pytest.raises(EmoHipError):
        o.interpolate_frames(x, 1)                              # k = 1
    with pytest.raises(EmoHipError):
        o.interpolate_frames(x, 2, method=7)
    n_in, n_out = x.numel(), 1 * 4 * 5 * 4 * 4
    buf = torch.zeros(n_in + n_out, device=DEV)
    buf[:n_in] = x.reshape(-1)
    xin = buf[:n_in].view(1, 4, 3, 4, 4)
    with pytest.raises(EmoHipError, match="overlaps"):
        o.interpolate_frames(xin, 2, out=buf[n_in - 4:n_in - 4 + n_out].view(1, 4, 5, 4, 4))
    need = o._lib.load().emo_interp_frames_workspace_bytes(1, 4, 3, 16)
    assert need > 0
    with pytest.raises(EmoHipError, match="workspace"):
        o.interpolate_frames(x, 2, workspace=torch.zeros(need - 1, device=DEV, dtype=torch.uint8))
    got = o.interpolate_frames(x, 2, workspace=torch.zeros(need, device=DEV, dtype=torch.uint8))
    assert torch.equal(got, o.interpolate_frames(x, 2))
    assert torch.equal(buf[:n_in], x.reshape(-1)) and float(buf[n_in:].abs().max()) == 0.0      # the refused calls launched nothing
