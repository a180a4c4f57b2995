"""GPU sweeps of csrc/elementwise.hip, the file every model pass starts and ends in: the layout pair (emo_ncfhw_to_rows /
emo_rows_to_ncfhw) over its tile edges, leading dimensions and the walk of a capped grid; the timestep sinusoid over dims, flip and both
entries; SiLU over its specials and trips; the fused sampler step over HW < 4, F = 1, misaligned bases, both grid-stride loops and its
counter-based noise; and the second trip of every other entry of the file.

The cases are the tables of tests/elementwise_sweep_cases.py; tests/test_host_logic.py redoes on the CPU the arithmetic each is named
for.  Data moves and single roundings compare BITS with the torch expression (permute, cast, one f32 add); arithmetic compares with f64 at
the tolerances the project already holds these kernels to (TOL of tests/test_gpu_kernels.py, the figures of
tests/test_gpu_sched_kernel.py).  Leading dimensions above the width and bases off a 16-byte boundary are reached through ctypes or
through views, whose neighbours are poisoned: they must be neither read into a result nor written."""
import ctypes as C
import functools

import pytest
import torch

from emote_hack_amd.synth import seeded_randn
from tests import elementwise_sweep_cases as E
from tests.test_gpu_kernels import DEV, DTYPES, TOL, close, ops, q       # noqa: F401  (TOL: the only parity tolerances used here)
from tests.test_gpu_sched_kernel import want_step
from tests.test_gpu_small_ops import untouched, wide_view

pytestmark = pytest.mark.gpu

NAN = float("nan")
LAYOUT_IDS = [E.layout_id(c) for c in E.LAYOUT]


def lib():
    from emote_hack_amd import _lib
    return _lib.load()


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def bits(t):
    """the bit patterns of a tensor, on the CPU: what torch.equal cannot tell apart (+0 / -0) or refuses to match (NaN) compares here"""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ layout pair
@functools.lru_cache(maxsize=2)
def layout_input(key):
    """f32 (B, C, F, H, W) of a case, NOT on any 16-bit grid (the cast rounds), the same for every dtype of the case"""
    c = E.LAYOUT[LAYOUT_IDS.index(key)]
    B, F, H, W = c["shape"]
    return seeded_randn((B, c["C"], F, H, W), 601) * 3


def layout_x(c, dtype):
    x = layout_input(E.layout_id(c)).clone()
    sp = E.rounding_specials(dtype)
    flat = x.view(-1)
    k = min(sp.numel(), flat.numel())
    flat[:k] = sp[:k]           # ties, the tie that rounds to infinity and its neighbours (as many as the case holds)
    return x


def to_rows(x, y, c, dtype, **over):
    """emo_ncfhw_to_rows with the case's arguments (ldo = Cpad), `over` replacing any of them"""
    B, F, H, W = c["shape"]
    a = dict(B=B, C=c["C"], F=F, H=H, W=W, Cpad=c["Cpad"], ldo=c["Cpad"])
    a.update(over)
    return lib().emo_ncfhw_to_rows(ptr(x), ptr(y), a["B"], a["C"], a["F"], a["H"], a["W"], a["Cpad"], a["ldo"], ops().dt(dtype), st())


def to_ncfhw(rows, y, c, dtype, **over):
    """emo_rows_to_ncfhw with the case's arguments and ldi = Cpad (rows of the padded layout), `over` replacing any of them"""
    B, F, H, W = c["shape"]
    a = dict(B=B, C=c["C"], F=F, H=H, W=W, ldi=c["Cpad"])
    a.update(over)
    return lib().emo_rows_to_ncfhw(ptr(rows), ptr(y), a["B"], a["C"], a["F"], a["H"], a["W"], a["ldi"], ops().dt(dtype), st())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", E.LAYOUT, ids=LAYOUT_IDS)
def test_ncfhw_to_rows_is_permute_and_cast_bit_for_bit(c, dtype):
    """emo_ncfhw_to_rows == x.permute(0, 2, 3, 4, 1).reshape(-1, C).to(dtype), every element, every bit; the pad columns [C, Cpad) are +0.
    Contiguous through ops.ncfhw_to_rows, and with ldo = Cpad + 16 into a buffer of NaN whose columns [Cpad, ldo) keep their bits."""
    o = ops()
    Cc, Cpad = c["C"], c["Cpad"]
    x = layout_x(c, dtype)
    want = x.permute(0, 2, 3, 4, 1).reshape(-1, Cc).to(dtype).contiguous()
    if dtype != torch.float32 and x.numel() >= 8:
        assert bool(torch.isinf(want[torch.isfinite(x.permute(0, 2, 3, 4, 1).reshape(-1, Cc))]).any())       # the tie above the largest value
    M = want.shape[0]
    xd = x.to(DEV)
    got = o.ncfhw_to_rows(xd, dtype, cpad=Cpad)
    assert got.dtype == dtype and tuple(got.shape) == (M, Cpad)
    assert same_bits(got[:, :Cc], want)
    assert not bool(bits(got[:, Cc:]).any())                  # +0, not -0, not a leftover
    ldo = Cpad + E.LAYOUT_LD_EXTRA
    buf = torch.full((M, ldo), NAN, device=DEV, dtype=dtype)
    before = bits(buf[:, Cpad:])
    assert to_rows(xd, buf, c, dtype, ldo=ldo) == 0
    torch.cuda.synchronize()
    assert same_bits(buf[:, :Cc], want)
    assert not bool(bits(buf[:, Cc:Cpad]).any())
    assert torch.equal(bits(buf[:, Cpad:]), before)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", E.LAYOUT, ids=LAYOUT_IDS)
def test_rows_to_ncfhw_is_widen_and_permute_bit_for_bit(c, dtype):
    """emo_rows_to_ncfhw == rows.float() permuted back, from contiguous rows and from a column view with ldi = C + 16 whose neighbours
    are NaN (none may reach the result); and the round trip of values already on the type's grid - infinities included - is the
    identity."""
    o = ops()
    B, F, H, W = c["shape"]
    Cc, Cpad = c["C"], c["Cpad"]
    rows = layout_x(c, dtype).permute(0, 2, 3, 4, 1).reshape(-1, Cc).to(dtype).contiguous()     # on the grid by construction
    want = rows.float().reshape(B, F, H, W, Cc).permute(0, 4, 1, 2, 3).contiguous()
    got = o.rows_to_ncfhw(rows.to(DEV), B, Cc, F, H, W)
    assert got.dtype == torch.float32 and same_bits(got, want)
    ldi = Cc + E.LAYOUT_LD_EXTRA
    buf = torch.full((rows.shape[0], ldi + 8), NAN, device=DEV, dtype=dtype)
    view = buf[:, 8:8 + Cc]                                    # starts on a 16-byte boundary in every type; ld = ldi + 8 > C
    view.copy_(rows.to(DEV))
    got = o.rows_to_ncfhw(view, B, Cc, F, H, W)
    assert not bool(torch.isnan(got).any()) and same_bits(got, want)
    # the round trip: rows of the padded layout back to (B, C, F, H, W)
    padded = o.ncfhw_to_rows(want.to(DEV), dtype, cpad=Cpad)
    assert same_bits(padded[:, :Cc], rows)
    assert same_bits(o.rows_to_ncfhw(padded[:, :Cc], B, Cc, F, H, W), want)


@pytest.mark.parametrize("c", [E.LAYOUT[0], E.LAYOUT[2]], ids=[LAYOUT_IDS[0], LAYOUT_IDS[2]])
def test_layout_refusals_launch_nothing(c):
    """Cpad < C, ldo < Cpad, ldi < C and a zero dimension are refused, and the poisoned output is as it was."""
    dtype = torch.bfloat16
    B, F, H, W = c["shape"]
    Cc, Cpad = c["C"], c["Cpad"]
    M = B * F * H * W
    x = seeded_randn((B, Cc, F, H, W), 602).to(DEV)
    rows = seeded_randn((M, Cpad), 603).to(DEV).to(dtype)
    out_rows = torch.full((M, Cpad), NAN, device=DEV, dtype=dtype)
    out_x = torch.full((B, Cc, F, H, W), NAN, device=DEV)
    br, bx = bits(out_rows), bits(out_x)
    n = 0
    for entry, over in E.layout_refusals(c):
        if entry == "to_rows":
            rc = to_rows(x, out_rows, c, dtype, **over)
        else:
            rc = to_ncfhw(rows, out_x, c, dtype, **over)
        assert rc != 0, (entry, over)
        n += 1
    torch.cuda.synchronize()
    assert n == 13 and torch.equal(bits(out_rows), br) and torch.equal(bits(out_x), bx)
    assert to_rows(x, out_rows, c, dtype) == 0 and to_ncfhw(rows, out_x, c, dtype) == 0       # the same calls, unspoilt
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out_x).any()) and not bool(torch.isnan(out_rows.float()).any())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("wa,wb", E.CONCAT_WIDTHS)
def test_concat_cols_is_torch_cat_bit_for_bit(dtype, wa, wb):
    o = ops()
    a, b = seeded_randn((E.CONCAT_M, wa), 611).to(dtype), seeded_randn((E.CONCAT_M, wb), 612).to(dtype)
    got = o.concat_cols(a.to(DEV), b.to(DEV))
    assert same_bits(got, torch.cat([a, b], 1))


# ------------------------------------------------------------------------------------------------ timestep sinusoid
def ts_check(ts, dim, flip, integral):
    """both entries (the int64 one on integral timesteps only) in every dtype against E.ts_reference"""
    o = ops()
    freqs = E.ts_freqs(dim).to(DEV)
    want = E.ts_reference(ts, dim, flip)
    tf = ts.float().to(DEV)
    f32 = o.timestep_embedding(tf, freqs, dim, flip, torch.float32)
    assert f32.dtype == torch.float32 and tuple(f32.shape) == (ts.shape[0], dim)
    err = (f32.cpu().double() - want).abs()
    print(f"timestep dim={dim} flip={flip} B={ts.shape[0]}: max |f32 - f64| = {float(err.max()):.3e}")
    torch.testing.assert_close(f32.cpu().double(), want, **E.TS_TOL)
    if dim % 2 == 1:
        assert not bool(bits(f32[:, -1]).any())               # the pad column: +0
    outs = {torch.float32: f32}
    for dtype in (torch.bfloat16, torch.float16):
        outs[dtype] = o.timestep_embedding(tf, freqs, dim, flip, dtype)
        assert same_bits(outs[dtype], f32.cpu().to(dtype)), dtype          # the store rounds the f32 value to nearest even
        if dim % 2 == 1:
            assert not bool(bits(outs[dtype][:, -1]).any())
    if integral:
        ti = ts.to(torch.int64).to(DEV)
        for dtype in DTYPES:
            assert same_bits(o.timestep_embedding(ti, freqs, dim, flip, dtype), outs[dtype]), dtype


@pytest.mark.parametrize("flip", E.TS_FLIPS)
@pytest.mark.parametrize("dim", E.TS_DIMS)
def test_timestep_embedding_dims_and_flip(dim, flip):
    """dim 2 (one frequency), odd dims (the zero pad column), both orders of [sin | cos]; integral timesteps through both entries, bit
    for bit the same; fractional ones through the f32 entry."""
    ts_check(torch.tensor(E.TS_INT, dtype=torch.int64), dim, flip, integral=True)
    ts_check(torch.tensor(E.TS_FRAC, dtype=torch.float32), dim, flip, integral=False)


@pytest.mark.parametrize("flip", E.TS_FLIPS)
def test_timestep_embedding_second_trip(flip):
    ts_check(E.ts_walk_timesteps(), E.TS_WALK["dim"], flip, integral=True)


# ------------------------------------------------------------------------------------------------ SiLU
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", E.SILU_SIZES)
def test_silu_specials_sizes_and_in_place(dtype, n):
    """x * sigmoid(x) in f64 on the quantised input; 0, -0, +-20, +-90, +-1e4 behind the random head (at those sizes the result is x or
    a zero / tiny negative, never NaN); y == x (in place, through ctypes) gives the bits of the out-of-place run."""
    o = ops()
    x = seeded_randn((n,), 621) * 4
    k = min(len(E.SILU_SPECIALS), n - 1)
    if k > 0:
        x[1:1 + k] = torch.tensor(E.SILU_SPECIALS[:k])
    x = q(x, dtype)
    xd = x.double()
    want = (xd * torch.sigmoid(xd)).float()
    xdev = x.to(DEV).to(dtype)
    got = o.silu(xdev)
    assert got.dtype == dtype and not bool(torch.isnan(got.float()).any())
    close(got, want, dtype)
    inplace = xdev.clone()
    assert lib().emo_silu(ptr(inplace), ptr(inplace), n, o.dt(dtype), st()) == 0
    torch.cuda.synchronize()
    assert same_bits(inplace, got)


# ------------------------------------------------------------------------------------------------ sampler step
@functools.lru_cache(maxsize=2)
def sched_inputs(n):
    """CPU inputs of an n-element step, shared by every variant of a case and never written: both noise_pred planes, latents, the ring,
    and the oracle's draw for (SCHED_SEED, SCHED_STEP)"""
    from oracle.scheduler_ref import counter_normal
    return seeded_randn((2, n), 1), seeded_randn((n,), 2) * 3, seeded_randn((4, n), 3), counter_normal(E.SCHED_SEED, E.SCHED_STEP, n)


def sched_counter(F):
    return torch.tensor([1.0 + (f % 3) for f in range(F)])


def sched_run(shape, gs, ring, c_noise, *, off=None, np_tail_nan=False, coef=None, seed=E.SCHED_SEED, step=E.SCHED_STEP):
    """one emo_sched_step on fresh device copies of the shared inputs -> (latents, lat_in, eps_out, ring) on the device.
    off = "lat" | "noise_pred" | "lat_in": that operand sits one f32 element behind a 16-byte boundary, inside a poisoned buffer whose
    other elements must survive (checked here).  np_tail_nan: noise_pred is the n-element head of a buffer whose tail is NaN."""
    C_, F, HW = shape
    n = C_ * F * HW
    np_, lat, hist, _ = sched_inputs(n)
    planes = 2 if gs > 1 else 1

    def place(t, name, poison):
        if off != name:
            return None, t.to(DEV, copy=True)
        buf = torch.full((t.numel() + 8,), poison, device=DEV)
        buf[1:1 + t.numel()] = t.reshape(-1)
        assert buf[1:].data_ptr() % 16 == 4
        return buf, buf[1:1 + t.numel()]

    if np_tail_nan:
        assert planes == 1
        nb = torch.full((2 * n,), NAN, device=DEV)
        nb[:n] = np_[0]
        np_buf, d_np = None, nb[:n]
    else:
        np_buf, d_np = place(np_[:planes].reshape(-1), "noise_pred", NAN)
    lat_buf, d_lat = place(lat, "lat", -3.0)
    in_buf, d_in = place(torch.full((n,), NAN), "lat_in", -3.0)
    d_hist = hist.to(DEV) if ring else None
    d_eps = torch.full((n,), NAN, device=DEV)
    r = E.SCHED_LMS if ring else E.SCHED_NO_RING
    k = dict(E.SCHED_COEF if coef is None else coef)
    ops().sched_step(d_np, sched_counter(F).to(DEV), d_lat, d_hist, d_in, C_=C_, F=F, HW=HW, guidance_scale=gs, a=k["a"], b=k["b"], c_x=k["c_x"],
                     c=r["c"], slot=r["slot"], c_noise=c_noise, s_next=k["s_next"], seed=seed, step=step, eps_out=d_eps)
    torch.cuda.synchronize()
    for buf in (lat_buf, in_buf):
        if buf is not None:
            assert float(buf[0]) == -3.0 and bool((buf[1 + n:] == -3.0).all())
    if np_buf is not None:
        assert bool(torch.isnan(np_buf[0])) and bool(torch.isnan(np_buf[1 + planes * n:]).all())
    return d_lat, d_in, d_eps, d_hist


def sched_check(shape, gs, ring, c_noise, **kw):
    C_, F, HW = shape
    n = C_ * F * HW
    np_, lat, hist, z = sched_inputs(n)
    r = E.SCHED_LMS if ring else E.SCHED_NO_RING
    want_x, want_d, want_eps, want_in = want_step(np_, sched_counter(F), lat, hist, C=C_, F=F, HW=HW, gs=gs, c=r["c"], slot=r["slot"],
                                                  c_noise=c_noise, z=z, **E.SCHED_COEF)
    d_lat, d_in, d_eps, d_hist = sched_run(shape, gs, ring, c_noise, **kw)
    for name, got, want in (("x'", d_lat, want_x), ("lat_in", d_in, want_in), ("eps", d_eps, want_eps)):
        err = (got.cpu().double() - want).abs()
        print(f"sched {shape} gs={gs} ring={ring} noise={c_noise} {name}: max err {float(err.max()):.3e} at |want| {float(want.abs().flatten()[err.argmax()]):.3e}")
        torch.testing.assert_close(got.cpu().double(), want, **E.SCHED_TOL)
    if ring:
        for k in range(4):      # the written slot holds d; every other slot is untouched
            if k == r["slot"][0]:
                torch.testing.assert_close(d_hist[k].cpu().double(), want_d, **E.SCHED_TOL)
            else:
                assert torch.equal(d_hist[k].cpu(), hist[k])
    return d_lat, d_in, d_eps, d_hist


@pytest.mark.parametrize("c_noise", [0.0, E.SCHED_C_NOISE])
@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("gs", E.SCHED_GUIDANCE)
@pytest.mark.parametrize("shape", E.SCHED_SMALL + E.SCHED_LARGE, ids=[E.sched_id(s) for s in E.SCHED_SMALL + E.SCHED_LARGE])
def test_sched_step_shapes_against_float64(shape, gs, ring, c_noise):
    """HW of 1, 2 and 3 on the float4 path (the frame changes, and wraps from F - 1 to 0, inside one vector), F = 1, and the second
    trip of the float4 loop and of the per-element loop: x', lat_in, eps_out and the ring against the f64 linear form.  With guidance
    1.0 noise_pred holds ONE plane, handed over as the head of a buffer whose tail is NaN: the cond plane is not read."""
    sched_check(shape, gs, ring, c_noise, np_tail_nan=(gs <= 1))


@pytest.mark.parametrize("which", E.SCHED_MISALIGNED)
@pytest.mark.parametrize("shape", E.SCHED_SMALL, ids=[E.sched_id(s) for s in E.SCHED_SMALL])
def test_sched_step_misaligned_base_gives_the_aligned_bits(shape, which):
    """One operand one f32 element off a 16-byte boundary sends the call down the per-element path: it computes the same expression per
    element, so every output has the bits of the aligned (float4) run of the same inputs; the elements around the operand survive."""
    for gs in E.SCHED_GUIDANCE:
        for ring in (False, True):
            for c_noise in (0.0, E.SCHED_C_NOISE):
                ref = sched_check(shape, gs, ring, c_noise)
                got = sched_check(shape, gs, ring, c_noise, off=which)
                for name, a, b in zip(("x'", "lat_in", "eps", "ring"), got, ref):
                    assert (a is None and b is None) or same_bits(a, b), (name, gs, ring, c_noise)


def test_sched_step_noise_is_the_oracles_counter_normal():
    """a = b = c_x = 0 and c_noise = 1 leave x' = z: the kernel's draw for two seeds and three steps against
    oracle.scheduler_ref.counter_normal; different (seed, step) pairs draw different numbers, the same pair the same."""
    from oracle.scheduler_ref import counter_normal
    shape = E.SCHED_DRAWS["shape"]
    n = shape[0] * shape[1] * shape[2]
    zero = dict(a=0.0, b=0.0, c_x=0.0, s_next=1.0)
    draws = {}
    for seed in E.SCHED_DRAWS["seeds"]:
        for step in E.SCHED_DRAWS["steps"]:
            x, x_in, _, _ = sched_run(shape, 7.5, False, 1.0, coef=zero, seed=seed, step=step)
            want = counter_normal(seed, step, n).double()
            err = (x.cpu().double() - want).abs()
            print(f"draw seed={seed} step={step}: max err {float(err.max()):.3e}")
            torch.testing.assert_close(x.cpu().double(), want, **E.SCHED_TOL)
            assert same_bits(x_in, x)
            draws[(seed, step)] = x.cpu()
    keys = list(draws)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert not torch.equal(draws[a], draws[b]), (a, b)
            assert float((draws[a] - draws[b]).abs().mean()) > 0.5            # E|z1 - z2| = 2 / sqrt(pi) for independent normals
    again, _, _, _ = sched_run(shape, 7.5, False, 1.0, coef=zero, seed=keys[0][0], step=keys[0][1])
    assert same_bits(again, draws[keys[0]])


# ------------------------------------------------------------------------------------------------ second trips of the other entries
def test_copy_cols_and_add_second_trip():
    """f32, 524672 vectors, source, second operand and destination all views with ld = 520: the copy is exact; a + 0.5 * b is ONE
    rounding whether or not the device contracts it (0.5 * b is exact), so it equals torch's f32 expression bit for bit."""
    o = ops()
    w = E.COPY_ADD_WALK
    M, Cc = w["M"], w["C"]
    a, b = seeded_randn((M, Cc), 631), seeded_randn((M, Cc), 632)
    abuf, av = wide_view(a, torch.float32, left=8, right=0)
    _, bv = wide_view(b, torch.float32, left=0, right=8)
    assert av.stride(0) == bv.stride(0) == w["ld"]
    ybuf = torch.full((M, w["ld"]), -3.0, device=DEV)
    o.copy_cols(av, ybuf, 4)
    assert same_bits(ybuf[:, 4:4 + Cc], a) and untouched(ybuf, 4, Cc, -3.0)
    sbuf, sv = wide_view(torch.zeros(M, Cc), torch.float32, left=8, right=0, poison=-3.0)
    o.add(av, bv, alpha=0.5, out=sv)
    assert same_bits(sv, a + 0.5 * b) and untouched(sbuf, 8, Cc, -3.0)


def test_add_periodic_second_trip_in_place():
    """bf16, 65541 rows of 64 channels in 9363 periods of 7 rows, in place: x + f[m % 7] added in f32 and rounded once."""
    o = ops()
    w = E.ADD_PERIODIC_WALK
    M, Cc, P = w["P"] * w["periods"], w["C"], w["P"]
    x, f = seeded_randn((M, Cc), 641).bfloat16(), seeded_randn((P, Cc), 642).bfloat16()
    want = (x.float().reshape(-1, P, Cc) + f.float()[None]).reshape(M, Cc).bfloat16()
    xd = x.to(DEV)
    got = o.add_periodic(xd, f.to(DEV))
    assert got.data_ptr() == xd.data_ptr() and same_bits(xd, want)


def test_convert_second_trip():
    o = ops()
    x = seeded_randn((E.CONVERT_WALK,), 651) * 3
    assert same_bits(o.convert(x.to(DEV), torch.bfloat16), x.bfloat16())


def test_accumulate_window_second_trip():
    """f32, 524400 elements, frames [2, -1, 0]: each accumulator element takes one f32 add; the skipped window position and frame 1 leave
    theirs alone; the counter is exactly [1, 0, 1]."""
    o = ops()
    w = E.ACCUMULATE_WALK
    nf, C4, HW, Ft = w["nf"], w["C"], w["HW"], w["F"]
    pred = seeded_randn((nf * HW, C4), 661)
    start = seeded_randn((C4, Ft, HW), 662)
    want = start.clone()
    for j, f in enumerate(w["frames"]):
        if f >= 0:
            want[:, f] += pred[j * HW:(j + 1) * HW].t()
    acc, cnt = start.to(DEV), torch.zeros(Ft, device=DEV)
    o.accumulate_window(pred.to(DEV), acc, cnt, torch.tensor(w["frames"], dtype=torch.int32, device=DEV), C_=C4, F=Ft, HW=HW, add_counter=True)
    assert same_bits(acc, want) and same_bits(acc[:, 1], start[:, 1])
    assert torch.equal(cnt.cpu(), torch.tensor(w["counter"]))
