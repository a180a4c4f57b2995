"""Sweeps of the dense tile GEMM (csrc/gemm_impl.h) over WINDOW operands: A is an overlapping row view of a (time, channel) sequence
with lda = s*C below K = k*C, the way emote_hack_amd/wav2vec2.py runs every 1-D convolution of the audio encoder - the feature
encoder's strided layers and the 16 per-group launches of the positional convolution (lda = cg, K = 128*cg, each writing a column
slice of one buffer).  tests/test_gpu_gemm_sweeps.py only builds lda >= K.  The case tables are tests/frontend_sweep_cases.py;
tests/test_host_logic.py checks on the CPU (emo_gemm_plan) that they reach every tile, both main loops and the split-K path, and that
the shapes wav2vec2-base runs at 1 s and 10 s of audio are among them.

The sequence x holds exactly T*C elements, T = (M - 1)*s + k, so the last window ends on its last element; a NaN guard block follows
(longer than K elements: with lda < K the loaders' buffer descriptors admit the first rows past M, whose requests - for accumulator
rows that are never stored - reach up to about K elements past the last window).  W is followed by a NaN guard,
the output is a column slice of a sentinel-filled buffer: every element outside the view must keep its bits.

Every case runs twice, as in the GEMM sweeps:
  * the exact probe: x one-hot per time step, W / bias multiples of 1/16 - out[m, n] = bias[n] + sum_j W[n, j*C + (m*s + j) % C] with
    every sum exact in all three dtypes (asserted on the CPU when the operands are built): the output must match BIT FOR BIT.  A
    descriptor sized M*lda, a dropped chunk, a window read one row off all show;
  * random operands against F.conv1d in f64 on inputs quantised to the compute dtype, at the TOL of tests/test_gpu_kernels.py."""
import pytest
import torch

from tests import frontend_sweep_cases as S
from tests.test_gpu_gemm_sweeps import DEV, IDS, bits, ops, sentinel, untouched
from tests.test_gpu_kernels import TOL

pytestmark = pytest.mark.gpu

BOTH = ("probe", "random")


def guarded(t, guard):
    """t on the device as a view of a flat buffer that holds exactly t's elements and then `guard` NaNs"""
    flat = torch.full((t.numel() + guard,), float("nan"), device=DEV, dtype=t.dtype)
    flat[:t.numel()] = t.reshape(-1).to(DEV)
    return flat[:t.numel()].view(t.shape)


def guard_len(K):
    return 2 * K + 4096


class Cache:
    """device operands per key; the cases that differ in tile / split / bias share them"""

    def __init__(self, build):
        self.build, self.d = build, {}

    def get(self, *key):
        if key not in self.d:
            if len(self.d) > 8:
                self.d.clear()
            self.d[key] = self.build(*key)
        return self.d[key]


def _win_dev(dtype, k, s, C, M, mode):
    op = S.win_operands(dtype, k, s, C, M, mode)
    x = guarded(op["x"].to(dtype), guard_len(k * C))
    return dict(op, a=torch.as_strided(x, (M, k * C), (s * C, 1)), w_d=guarded(op["w"].to(dtype), 4096), bias_d=op["bias"].to(DEV))


def _pos_dev(dtype, kp, cg, T, mode):
    op = S.pos_operands(dtype, kp, cg, T, mode)
    G = S.POS_G
    xp = torch.zeros(G, T + 2 * (kp // 2), cg)
    xp[:, kp // 2:kp // 2 + T] = op["h"].view(T, G, cg).permute(1, 0, 2)          # group-major, zero-padded in time
    xp = guarded(xp.to(dtype), guard_len(kp * cg))
    return dict(op, a=[torch.as_strided(xp[gi], (T, kp * cg), (cg, 1)) for gi in range(G)],
                w_d=[guarded(op["w"][gi].to(dtype), 4096) for gi in range(G)],
                bias_d=[op["bias"][gi * cg:(gi + 1) * cg].contiguous().to(DEV) for gi in range(G)])


WIN, POS = Cache(_win_dev), Cache(_pos_dev)


def launch(c, a, w, bias, ldc, c0, split, rows_behind=3):
    """one emo_gemm into columns [c0, c0 + N) of a sentinel (M + rows_behind, ldc) buffer, run twice when split (a NaN workspace in
    front of each): -> the (M, N) result as f32 on the CPU"""
    o, dtype, M, N = ops(), c["dtype"], c["M"], c["N"]
    outs = []
    for _rep in range(2 if split > 1 else 1):
        kw = dict(workspace=torch.full((split * M * N,), float("nan"), device=DEV, dtype=torch.float32)) if split > 1 else {}
        buf = sentinel((M + rows_behind, ldc), dtype)
        view = buf[:M, c0:c0 + N]
        o.gemm(a, w, bias, out=view, split_k=split, tile=c["tile"], **kw)
        keep = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
        keep[:M, c0:c0 + N] = False
        assert untouched(buf, keep), f"{c}: wrote outside the M x N view"
        outs.append(view.float().cpu())
    if len(outs) == 2:
        assert torch.equal(bits(outs[0]), bits(outs[1])), f"{c}: split-K is not deterministic"
    return outs[0]


def check(c, mode, got, y64):
    dtype = c["dtype"]
    if mode == "probe":
        want = y64.to(dtype).float()
        bad = got != want
        assert not bool(bad.any()), (f"{c}: exact probe, {int(bad.sum())} of {bad.numel()} elements differ, first at "
                                     f"{bad.nonzero()[0].tolist()}: got {got[bad][0].item()} want {want[bad][0].item()}")
    else:
        try:
            torch.testing.assert_close(got, y64.float(), **TOL[dtype])
        except AssertionError as e:
            raise AssertionError(f"{c}: {e}") from None


# ---- A. the strided layers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", S.WIN_KS, ids=lambda ks: f"k{ks[0]}s{ks[1]}")
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_window_rows_probe_and_random(dtype, ks):
    """(k, s) x C in {V, BK/2 + V, 2 BK} x M in {1, 300} x tile hints 0..7 x split_k in {1, planned, 3} x bias: the window view's rows
    overlap (lda < K; lda == K for (2, 2)), the descriptor must span (M - 1)*lda + K elements and not one more row of x than exists."""
    for c in S.win_cases(dtype, *ks):
        g = S.win_geometry(c)
        split = c["split_k"] if c["split_k"] is not None else S.win_plan(c)[4]
        for mode in BOTH:
            op = WIN.get(dtype, c["k"], c["s"], c["C"], c["M"], mode)
            got = launch(c, op["a"], op["w_d"], op["bias_d"] if c["bias"] else None, g["ldc"], g["c0"], max(split, 1))
            check(c, mode, got, op["y0_bias"] if c["bias"] else op["y0"])


# ---- A'. the positional convolution ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kp", S.POS_KP)
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_grouped_positional_conv_probe_and_random(dtype, kp):
    """One launch per group over xp (G, T + 2 (kp // 2), cg): lda = cg, K = kp*cg, N = cg, a bias, into out[:, gi*cg : (gi + 1)*cg] of a
    (T, G*cg) sentinel buffer - after each single launch the other groups' columns still hold the sentinel.  Against
    F.conv1d(groups=G, padding=kp // 2)[..., :T] in f64; the last group's last window ends on (kp odd) or one step before (kp even)
    the last element of xp."""
    for c in (c for c in S.pos_cases(dtype) if c["kp"] == kp):
        cg, G = c["cg"], c["G"]
        split = c["split_k"] if c["split_k"] is not None else S.pos_plan(c)[4]
        for mode in BOTH:
            op = POS.get(dtype, kp, cg, c["T"], mode)
            got = torch.cat([launch(c, op["a"][gi], op["w_d"][gi], op["bias_d"][gi], G * cg, gi * cg, max(split, 1)) for gi in range(G)], 1)
            check(c, mode, got, op["y"])
