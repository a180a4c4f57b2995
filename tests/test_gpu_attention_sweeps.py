"""GPU parity sweeps of emo_attention / emo_temporal_attention over what their dispatch code can pick: every admissible head dim
(= every (head-dim class, loader rounds, ring depth) instantiation, every residue of the denominator row), the key-count edges of the
masked tile body, the ring schedule over (tiles of segment 0, tiles of the bank segment), the resident and the causal walk, strided
operands, and for the temporal kernels every frame count, partial channel blocks, the per-wave item walk, the generic kernel on the
2-byte types and head counts that do not halve.  tests/test_host_logic.py checks on the CPU (emo_attention_plan) that the shapes
used here reach every instantiation.

The reference is a plain torch CPU softmax attention in f32 on the same quantised inputs; all elements are compared at the
tolerances of tests/test_gpu_kernels.py."""
import ctypes as C

import pytest
import torch

from emote_hack_amd.synth import seeded_randn
from tests import attention_sweep_cases as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {torch.float32: dict(rtol=1e-3, atol=1e-4), torch.bfloat16: dict(rtol=3e-2, atol=3e-2), torch.float16: dict(rtol=5e-3, atol=5e-3)}
DTYPES = S.DTYPES
TWO_BYTE = [torch.bfloat16, torch.float16]
NAN = float("nan")


def ops():
    from emote_hack_amd import ops as o
    return o


def q(t, dtype):
    """quantise a CPU fp32 tensor to the compute dtype's grid (inputs are identical on both sides)."""
    return t.to(dtype).float()


def close(got, ref, dtype, what=""):
    tol = TOL[dtype]
    torch.testing.assert_close(got.float().cpu(), ref, rtol=tol["rtol"], atol=tol["atol"], msg=lambda m: f"{what}: {m}")


def heads_of(t, heads, d):
    return t.reshape(t.shape[0], -1, heads, d).permute(0, 2, 1, 3)     # (B, L, heads*d) -> (B, heads, L, d)


def attn_ref(qq, kk, vv, heads, d, scale, causal=False):
    """softmax(q k^T * scale) v per (batch row, head): (B, Lq, C), (B, Lk, C), (B, Lk, C) -> (B * Lq, C), f32."""
    s = torch.matmul(heads_of(qq, heads, d), heads_of(kk, heads, d).transpose(-1, -2)) * scale
    if causal:
        L = s.shape[-1]
        s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float("-inf"))
    o_ = torch.matmul(s.softmax(-1), heads_of(vv, heads, d))
    return o_.permute(0, 2, 1, 3).reshape(qq.shape[0] * qq.shape[1], heads * d)


def vt_padded(v, extra=0):
    """V^T (rows, C, ld) of v (rows, L, C): ld = L rounded up to 8 (+ extra), NaN in the padding."""
    rows, L, C_ = v.shape
    ld = (L + 7) // 8 * 8 + extra
    vt = torch.full((rows, C_, ld), NAN)
    vt[:, :, :L] = v.permute(0, 2, 1)
    return vt


def dv(t, dtype):
    return t.to(DEV).to(dtype)


def two_segment(dtype, d, *, B, heads, Lq, Lk0, Lk1, first, seed, seg0_div=1, bank_rows=1, select="div", vt_extra=0, what=""):
    """One launch over [segment 0 of the batch row] ++ [a bank row, for batch rows >= first] against the reference.  The bank has
    `bank_rows` materialised rows; select = "div": batch row b reads row b - seg1_skip (seg1_div 1; seg1_skip 1 wherever batch row 0
    skips the bank: its row was never materialised), "word": every batch row reads the row named by the device word (the last one)."""
    o = ops()
    C_, scale = heads * d, d ** -0.5
    qq = q(seeded_randn((B, Lq, C_), seed), dtype)
    kk, vv = (q(seeded_randn((B // seg0_div, Lk0, C_), seed + i), dtype) for i in (1, 2))
    kw = {}
    ref_k, ref_v = kk.repeat_interleave(seg0_div, 0), vv.repeat_interleave(seg0_div, 0)
    if Lk1:
        bk, bv = (q(seeded_randn((bank_rows, Lk1, C_), seed + i), dtype) for i in (3, 4))
        if select == "div":
            skip = min(first, 1)
            assert bank_rows >= B - skip
            rows = [b - skip for b in range(first, B)]
            kw = dict(seg1_div=1, seg1_first_batch=first, seg1_skip=skip)
        else:
            rows = [bank_rows - 1] * (B - first)
            kw = dict(seg1_div=B, seg1_first_batch=first, seg1_row=torch.tensor([bank_rows - 1], dtype=torch.int32, device=DEV))
        kw.update(k1=dv(bk.reshape(-1, C_), dtype), v1t=dv(vt_padded(bv, vt_extra), dtype), Lk1=Lk1)
        ref = attn_ref(qq[first:], torch.cat([ref_k[first:], bk[rows]], 1), torch.cat([ref_v[first:], bv[rows]], 1), heads, d, scale)
        if first:
            ref = torch.cat([attn_ref(qq[:first], ref_k[:first], ref_v[:first], heads, d, scale), ref])
    else:
        ref = attn_ref(qq, ref_k, ref_v, heads, d, scale)
    got = o.attention(dv(qq.reshape(-1, C_), dtype), dv(kk.reshape(-1, C_), dtype), dv(vt_padded(vv, vt_extra), dtype), Lk0, B=B, Lq=Lq,
                      heads=heads, d=d, scale=scale, seg0_div=seg0_div, **kw)
    close(got, ref, dtype, what or f"d={d} Lq={Lq} Lk={Lk0}+{Lk1} {select}")
    return got, ref


# ------------------------------------------------------------------ a. every head dim, streaming, two segments
@pytest.mark.parametrize("dtype,d", S.ALL_DIMS)
def test_attention_every_head_dim_streaming(dtype, d):
    """B * heads = 6 (plain block order), head offsets head * d off the 32-element grid, 205 + 77 keys: a V^T chunk straddles Lk in
    one of the segments for every dtype; batch row 0 is a one-segment row of the same launch."""
    s = S.STREAM
    assert S.plan(dtype, d, B=s["B"], Lq=s["Lq"], Lk0=s["Lk0"], heads=s["heads"], Lk1=s["Lk1"])[3] == 1
    two_segment(dtype, d, B=s["B"], heads=s["heads"], Lq=s["Lq"], Lk0=s["Lk0"], Lk1=s["Lk1"], first=s["seg1_first_batch"], seed=100 + d,
                bank_rows=2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_xcd_block_orders(dtype):
    """The same with B * heads a multiple of 8: the round-robin block order (no bank-less rows in front) and the reversed one (rows
    without the bank segment first in memory, last in the launch), at one head dim per (class, loader rounds)."""
    s, seen = S.STREAM_ORDERED, set()
    for d in S.head_dims(dtype):
        pl = S.plan(dtype, d, B=s["B"], Lq=s["Lq"], Lk0=s["Lk0"], heads=s["heads"], Lk1=s["Lk1"])
        if pl[:2] in seen:
            continue
        seen.add(pl[:2])
        assert pl[3] == 1
        for first in (2, 0):
            two_segment(dtype, d, B=s["B"], heads=s["heads"], Lq=s["Lq"], Lk0=s["Lk0"], Lk1=s["Lk1"], first=first, seed=300 + d, bank_rows=4)
    assert len(seen) >= 6


# ------------------------------------------------------------------ b. every head dim, resident walk
@pytest.mark.parametrize("dtype,d", S.ALL_DIMS)
def test_attention_every_head_dim_resident(dtype, d):
    """One ragged KV tile kept in its slot while a block walks 2 (Lq 300: the last group holds one tile) or 4 (Lq 520) q tiles;
    context per batch row and shared by 4.  The variant is asserted through the plan query, not trusted."""
    o = ops()
    r = S.RESIDENT
    B, heads, Lk = r["B"], r["heads"], r["Lk0"]
    C_, scale = heads * d, d ** -0.5
    q_all = q(seeded_randn((B, max(S.RESIDENT_LQ), C_), 500 + d), dtype)
    kk, vv = (q(seeded_randn((B, Lk, C_), 501 + d + i), dtype) for i in (0, 1))
    for Lq, q_rep in S.RESIDENT_LQ.items():
        assert S.plan(dtype, d, B=B, Lq=Lq, Lk0=Lk, heads=heads)[3] == q_rep
        qq = q_all[:, :Lq].contiguous()
        for div in S.RESIDENT_DIV:
            k_, v_ = kk[:B // div], vv[:B // div]
            ref = attn_ref(qq, k_.repeat_interleave(div, 0), v_.repeat_interleave(div, 0), heads, d, scale)
            got = o.attention(dv(qq.reshape(-1, C_), dtype), dv(k_.reshape(-1, C_), dtype), dv(vt_padded(v_), dtype), Lk, B=B, Lq=Lq, heads=heads,
                              d=d, scale=scale, seg0_div=div)
            close(got, ref, dtype, f"d={d} Lq={Lq} div={div}")


# ------------------------------------------------------------------ c. causal
@pytest.mark.parametrize("dtype,d", S.ALL_DIMS)
def test_attention_every_head_dim_causal(dtype, d):
    """Causal self-attention at 77 (two tiles, the second ragged) and 200 keys (four tiles, two q tiles), and the resident causal walk
    wherever the plan reports it (the three tiles of L = 150 fit the ring).  Reference: masked softmax."""
    o = ops()
    c, cr = S.CAUSAL, S.CAUSAL_RESIDENT
    shapes = [(c["B"], c["heads"], L, False) for L in S.CAUSAL_L]
    if S.plan(dtype, d, B=cr["B"], Lq=cr["L"], Lk0=cr["L"], heads=cr["heads"], causal=True)[3] > 1:
        shapes.append((cr["B"], cr["heads"], cr["L"], True))
    for B, heads, L, resident in shapes:
        pl = S.plan(dtype, d, B=B, Lq=L, Lk0=L, heads=heads, causal=True)
        assert pl[4] == 1 and (pl[3] > 1) == resident
        C_, scale = heads * d, d ** -0.5
        qq, kk, vv = (q(seeded_randn((B, L, C_), 700 + d + i), dtype) for i in range(3))
        ref = attn_ref(qq, kk, vv, heads, d, scale, causal=True)
        got = o.attention(dv(qq.reshape(-1, C_), dtype), dv(kk.reshape(-1, C_), dtype), dv(vt_padded(vv), dtype), L, B=B, Lq=L, heads=heads, d=d,
                          scale=scale, causal=True)
        close(got, ref, dtype, f"causal d={d} L={L} B={B}")


# ------------------------------------------------------------------ d. key-count and query-count edges
@pytest.mark.parametrize("behind", [False, True])
@pytest.mark.parametrize("d", S.EDGE_DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_key_and_query_count_edges(dtype, d, behind):
    """The boundaries of the masked tile body (Lk % 64 in {1, 32, 33, 63, 0}, chunks straddling Lk) with the ragged tile as the only
    segment or as the bank segment behind 128 keys, at 1, 33 and 129 query rows.  V^T carries NaN behind every Lk (a whole spare
    chunk too).  One key: the output is that key's V row."""
    o = ops()
    e = S.EDGE
    B, heads = e["B"], e["heads"]
    C_, scale = heads * d, d ** -0.5
    for Lk in S.EDGE_LK:
        for Lq in S.EDGE_LQ:
            seed = 900 + 7 * Lk + Lq
            if behind:
                two_segment(dtype, d, B=B, heads=heads, Lq=Lq, Lk0=e["Lk0_front"], Lk1=Lk, first=0, seed=seed, bank_rows=B, vt_extra=8)
            else:
                got, _ = two_segment(dtype, d, B=B, heads=heads, Lq=Lq, Lk0=Lk, Lk1=0, first=0, seed=seed, vt_extra=8)
                if Lk == 1:
                    vrow = q(seeded_randn((B, 1, C_), seed + 2), dtype)
                    close(got, vrow.expand(B, Lq, C_).reshape(B * Lq, C_), dtype, f"one key d={d} Lq={Lq}")


# ------------------------------------------------------------------ e. ring schedule matrix
@pytest.mark.parametrize("tiles0", S.RING_TILES0)
@pytest.mark.parametrize("dtype,d", S.RING)
def test_attention_ring_schedule_matrix(dtype, d, tiles0):
    """(tiles of segment 0) x (tiles of the bank segment) on each ring depth: the prologue requests, the special tiles and the switch of
    descriptors at the first bank tile all depend on that pair.  Each segment ends once on a tile boundary and once ragged; batch
    rows 0-1 have one segment, 2-3 two; the bank row (of 3) is picked by seg1_div / seg1_skip and by the device word."""
    B, heads, Lq = 4, 2, 130
    for tiles1 in S.RING_TILES1:
        for Lk0, Lk1 in ((tiles0 * 64, tiles1 * 64 - 27), (tiles0 * 64 - 19, tiles1 * 64)):
            Lk1 = max(Lk1, 0)
            for select in (("div", "word") if tiles1 else ("div",)):
                two_segment(dtype, d, B=B, heads=heads, Lq=Lq, Lk0=Lk0, Lk1=Lk1, first=2, seed=1100 + 10 * tiles0 + tiles1, bank_rows=3, select=select)


# ------------------------------------------------------------------ f. strided operands and untouched bytes
def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _window_check(buf, r0, c0, M, C_, ref, dtype, sentinel, what):
    """rows [r0, r0 + M) x columns [c0, c0 + C_) of buf match ref; everything else still holds the sentinel, bit for bit."""
    host = buf.cpu()
    close(host[r0:r0 + M, c0:c0 + C_], ref, dtype, what)
    outside = torch.ones(host.shape, dtype=torch.bool)
    outside[r0:r0 + M, c0:c0 + C_] = False
    want = _bits(torch.full((1,), sentinel, dtype=dtype))[0]
    assert bool((_bits(host)[outside] == want).all()), f"{what}: bytes outside the output window were written"


@pytest.mark.parametrize("d", [24, 80])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_strided_operands_and_untouched_bytes(dtype, d):
    """q and k as column views of one (M, 2C + 16) buffer (spare columns NaN), out as a window of a larger sentinel-filled buffer
    (ldo = C + 16): the leading dims are honoured on both sides and nothing outside the window is written."""
    o = ops()
    B, heads, L = 2, 3, 150
    C_, M, scale = heads * d, B * L, d ** -0.5
    qq, kk, vv = (q(seeded_randn((B, L, C_), 1300 + d + i), dtype) for i in range(3))
    qk = torch.full((M, 2 * C_ + 16), NAN)
    qk[:, :C_], qk[:, C_:2 * C_] = qq.reshape(M, C_), kk.reshape(M, C_)
    qk = dv(qk, dtype)
    sentinel = 123.0
    buf = torch.full((M + 8, C_ + 16), sentinel, device=DEV, dtype=dtype)
    view = buf[4:4 + M, 8:8 + C_]
    ret = o.attention(qk[:, :C_], qk[:, C_:2 * C_], dv(vt_padded(vv), dtype), L, B=B, Lq=L, heads=heads, d=d, scale=scale, out=view)
    assert ret.data_ptr() == view.data_ptr() and ret.stride(0) == C_ + 16
    _window_check(buf, 4, 8, M, C_, attn_ref(qq, kk, vv, heads, d, scale), dtype, sentinel, f"strided d={d}")


def temporal_ref(qkv, B, Fr, HW, heads, d, scale):
    """(B * F * HW, 3C) q|k|v rows -> (B * F * HW, C): attention over the frames of every (batch row, pixel, head)."""
    t = qkv.reshape(B, Fr, HW, 3, heads, d).permute(3, 0, 2, 4, 1, 5)   # (3, B, HW, heads, F, d)
    s = torch.matmul(t[0], t[1].transpose(-1, -2)) * scale
    return torch.matmul(s.softmax(-1), t[2]).permute(0, 3, 1, 2, 4).reshape(B * Fr * HW, heads * d)


@pytest.mark.parametrize("d", [24, 80])
@pytest.mark.parametrize("dtype", DTYPES)
def test_temporal_attention_strided_operands_and_untouched_bytes(dtype, d):
    """ldqkv = 3C + 16 (NaN in the spare columns), ldo = C + 16 into a sentinel-filled buffer, at 12 and 20 frames."""
    o = ops()
    B, HW, heads = 2, 5, 3
    C_, scale = heads * d, d ** -0.5
    for Fr in (12, 20):
        M = B * Fr * HW
        qkv = q(seeded_randn((M, 3 * C_), 1400 + d + Fr), dtype)
        wide = torch.full((M, 3 * C_ + 16), NAN)
        wide[:, :3 * C_] = qkv
        sentinel = -77.0
        buf = torch.full((M + 8, C_ + 16), sentinel, device=DEV, dtype=dtype)
        view = buf[4:4 + M, 8:8 + C_]
        ret = o.temporal_attention(dv(wide, dtype)[:, :3 * C_], B, Fr, HW, heads, d, scale, out=view)
        assert ret.data_ptr() == view.data_ptr()
        _window_check(buf, 4, 8, M, C_, temporal_ref(qkv, B, Fr, HW, heads, d, scale), dtype, sentinel, f"temporal strided d={d} F={Fr}")


# ------------------------------------------------------------------ g. temporal attention
def temporal_case(dtype, B, Fr, HW, heads, d, seed, item_scale=False):
    o = ops()
    C_, scale = heads * d, d ** -0.5
    qkv = seeded_randn((B * Fr * HW, 3 * C_), seed)
    if item_scale:
        # item = (batch row * HW + pixel) * heads + head: its V is scaled by a factor that differs from the items the same wave
        # walks before and after it (item +- 8192: 8192 % 3 = 2), so a stale V image is far off
        fac = torch.tensor([1.0, -1.5, 2.0])[torch.arange(B * HW * heads) % 3].reshape(B, 1, HW, heads, 1)
        qkv.view(B, Fr, HW, 3, heads, d)[:, :, :, 2] *= fac
    qkv = q(qkv, dtype)
    got = o.temporal_attention(dv(qkv, dtype), B, Fr, HW, heads, d, scale)
    close(got, temporal_ref(qkv, B, Fr, HW, heads, d, scale), dtype, f"temporal F={Fr} d={d} heads={heads} HW={HW}")


@pytest.mark.parametrize("d", [8, 24, 40, 64, 80, 160])
@pytest.mark.parametrize("dtype", DTYPES)
def test_temporal_attention_every_frame_count(dtype, d):
    """F = 1..32: both MFMA block counts and every pad-frame mask, partial k-steps (d % 32) and channel blocks (d % 16); in f32 the
    generic kernel with F off the 3 x 3 score blocks, 5 pixels against P pixels per block and a head count that does not halve."""
    for Fr in range(1, 33):
        temporal_case(dtype, 2, Fr, 5, 3, d, 1500 + Fr)


@pytest.mark.parametrize("Fr", [12, 20])
@pytest.mark.parametrize("dtype", TWO_BYTE)
def test_temporal_attention_item_walk(dtype, Fr):
    """16432 (batch row, pixel, head) items on a grid capped at 2048 blocks x 4 waves: every wave walks two or three items over
    the same LDS V image and the last round is ragged."""
    temporal_case(dtype, 2, Fr, 1027, 8, 40, 1600 + Fr, item_scale=True)


@pytest.mark.parametrize("Fr,d", [(24, 256), (32, 264)])
@pytest.mark.parametrize("dtype", TWO_BYTE)
def test_temporal_attention_generic_kernel_two_byte(dtype, Fr, d):
    """Head dims whose four wave-private V images do not fit the MFMA kernel's LDS (d = 256 above 16 frames) or lie above its range."""
    temporal_case(dtype, 2, Fr, 5, 2, d, 1700 + Fr)


@pytest.mark.parametrize("heads,d,Fr", [(5, 64, 16), (6, 160, 24), (3, 160, 32), (7, 80, 32), (12, 160, 24), (9, 64, 20), (10, 128, 17)])
def test_temporal_attention_f32_head_counts_that_do_not_halve(heads, d, Fr):
    """f32 (the validation mode) on head counts whose halving stops at an odd number of heads per block too large for LDS: the
    launch steps down to a divisor that fits (one head per block always does here) - the 2-byte path serves all of these."""
    temporal_case(torch.float32, 2, Fr, 5, heads, d, 1800 + heads)
    temporal_case(torch.bfloat16, 2, Fr, 5, heads, d, 1800 + heads)


@pytest.mark.parametrize("dtype", DTYPES)
def test_temporal_attention_refusals_launch_nothing(dtype):
    from emote_hack_amd import _lib
    from emote_hack_amd.ops import dt
    lib = _lib.load()
    B, HW, heads, d = 1, 4, 2, 16
    C_ = heads * d
    qkv = torch.zeros(B * 33 * HW, 3 * C_, device=DEV, dtype=dtype)
    out = torch.full((B * 33 * HW, C_), 5.0, device=DEV, dtype=dtype)
    call = lambda Fr, d_, ldo: lib.emo_temporal_attention(C.c_void_p(qkv.data_ptr()), 3 * C_, C.c_void_p(out.data_ptr()), ldo, B, Fr, HW, heads, d_,
                                                          0.25, dt(dtype), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call(33, d, C_) != 0                 # more than 32 frames
    assert call(8, d + 2, C_) != 0              # d % V
    assert call(8, d, C_ - 8) != 0              # ldo < C
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    assert call(8, d, C_) == 0
    torch.cuda.synchronize()
    assert bool((out[:B * 8 * HW] == 0.0).all()) and bool((out[B * 8 * HW:] == 5.0).all())
