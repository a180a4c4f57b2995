"""emo_sched_step (the fused CFG + scheduler step) against a float64 torch evaluation of its linear form and, for DDIM / DDPM, against
the bits of the kernel it replaced; the f32 timestep embedding against the int64 entry and the oracle."""
from __future__ import annotations

import os

import pytest
import torch

from emote_hack_amd.synth import seeded_randn

pytestmark = pytest.mark.gpu
DEV = "cuda"


def want_step(np_, counter, lat, hist, *, C, F, HW, gs, a, b, c_x, c, slot, c_noise, s_next, z):
    n = C * F * HW
    cnt = counter.double().view(1, F, 1).expand(C, F, HW).reshape(-1)
    eps = np_[0].double() / cnt
    if gs > 1:
        eps = eps + gs * (np_[1].double() / cnt - eps)
    x = lat.double()
    d = a * x + b * eps
    out = c_x * x + c[0] * d
    for k in range(1, 4):
        if slot[k] >= 0:
            out = out + c[k] * hist[slot[k]].double()
    if c_noise:
        out = out + c_noise * z.double()
    return out, d, eps, s_next * out


CASES = [   # (C, F, HW, gs, n_terms, slot0, with lat_in, with eps_out, noise)
    (4, 3, 64, 7.5, 1, -1, True, True, 0.0),      # Euler
    (4, 3, 64, 1.0, 2, 1, True, False, 0.0),      # DPM++ 2M, no CFG
    (4, 5, 63, 7.5, 4, 3, False, True, 0.0),      # LMS order 4, HW % 4 != 0 (the frame changes inside a float4)
    (4, 2, 7, 7.5, 4, 0, True, True, 0.0),        # ring wrap: slot 0 written, 3 / 2 / 1 read
    (3, 3, 5, 7.5, 3, 2, True, True, 0.0),        # n % 4 != 0: the per-element path
    (4, 3, 64, 7.5, 1, -1, True, True, 0.7),      # Euler-a
    (3, 2, 9, 2.0, 2, 0, False, False, 0.3),      # noise on the per-element path
]


@pytest.mark.parametrize("C,F,HW,gs,nt,slot0,use_in,use_eps,c_noise", CASES)
def test_sched_step_against_float64(C, F, HW, gs, nt, slot0, use_in, use_eps, c_noise):
    from emote_hack_amd import ops
    from oracle.scheduler_ref import counter_normal
    n = C * F * HW
    nbr = 2 if gs > 1 else 1
    np_ = seeded_randn((nbr, n), 1)
    counter = torch.tensor([1.0 + (f % 3) for f in range(F)])
    lat = seeded_randn((n,), 2) * 3
    hist = seeded_randn((4, n), 3)
    slot = [slot0] + [((slot0 if slot0 >= 0 else 0) - k) % 4 if k < nt else -1 for k in range(1, 4)]
    c = [0.9, -0.4, 0.2, -0.05][:nt] + [0.0] * (4 - nt)
    kw = dict(C=C, F=F, HW=HW, gs=gs, a=0.8, b=-0.3, c_x=0.95, c=c, slot=slot, c_noise=c_noise, s_next=0.37)
    z = counter_normal(11, 4, n)
    want_x, want_d, want_eps, want_in = want_step(np_, counter, lat, hist, z=z, **kw)
    d_np, d_cnt, d_lat, d_hist = np_.to(DEV), counter.to(DEV), lat.to(DEV), hist.to(DEV)
    d_in = torch.full((n,), float("nan"), device=DEV) if use_in else None
    d_eps = torch.full((n,), float("nan"), device=DEV) if use_eps else None
    ops.sched_step(d_np, d_cnt, d_lat, d_hist, d_in, C_=C, F=F, HW=HW, guidance_scale=gs, a=0.8, b=-0.3, c_x=0.95, c=c, slot=slot,
                   c_noise=c_noise, s_next=0.37, seed=11, step=4, eps_out=d_eps)
    torch.cuda.synchronize()
    tol = dict(rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(d_lat.cpu().double(), want_x, **tol)
    if use_in:
        torch.testing.assert_close(d_in.cpu().double(), want_in, **tol)
    if use_eps:
        torch.testing.assert_close(d_eps.cpu().double(), want_eps, **tol)
    for k in range(4):   # the written slot holds d; every other slot is untouched
        if k == slot0:
            torch.testing.assert_close(d_hist[k].cpu().double(), want_d, **tol)
        else:
            assert torch.equal(d_hist[k].cpu(), hist[k])


def test_sched_scale_only():
    from emote_hack_amd import ops
    for C, F, HW in ((4, 3, 64), (3, 3, 5)):
        lat = seeded_randn((C * F * HW,), 4).to(DEV)
        out = torch.empty_like(lat)
        ops.sched_scale(lat, out, C_=C, F=F, HW=HW, s=0.25)
        torch.testing.assert_close(out, lat * 0.25, rtol=0, atol=0)


@pytest.mark.parametrize("C,F,HW", [(4, 3, 64), (3, 3, 5)])
def test_ddim_ddpm_plans_give_the_retired_cfg_step_bits(C, F, HW):
    """DDIM (eta 0 and 0.5) and DDPM (t > 0 and t = 0) at guidance 7.5 and 1.0, through emo_sched_step with the plans of
    DDIMScheduler / DDPMScheduler.step_plan: latents and eps_out equal, bit for bit, what emo_cfg_step (cfg_step_kernel, the
    DDIM / DDPM step before every scheduler ran on emo_sched_step) returned for the same inputs at commit cae0c69 on an MI355X
    (tests/golden/sched_ddim_ddpm.safetensors).  (4, 3, 64) takes the float4 path, (3, 3, 5) the per-element one."""
    import json
    from safetensors import safe_open
    from emote_hack_amd import ops
    from emote_hack_amd.scheduler import DDIMScheduler, DDPMScheduler
    from tests import cases
    key, n = f"{C}x{F}x{HW}", C * F * HW
    with safe_open(os.path.join(cases.GOLDEN_DIR, "sched_ddim_ddpm.safetensors"), "pt") as f:
        meta = f.metadata()
        g = {k: f.get_tensor(k) for k in f.keys() if k.startswith(key + "/")}
    np_, counter = g[f"{key}/noise_pred"].to(DEV), g[f"{key}/counter"].to(DEV)
    for name, case in json.loads(meta["cases"]).items():
        sch = DDIMScheduler(eta=case["eta"]) if name.startswith("ddim") else DDPMScheduler()
        sch.set_timesteps(case["steps"])
        si = case["si"]
        assert sch.timesteps[si] == case["t"] and sch.history == 0
        p = sch.step_plan(si)
        assert (p.c_x, p.c[0], p.c_noise) == (case["c_x"], case["c_eps"], case["c_noise"])   # the recorded coefficients
        for gs in json.loads(meta["guidance_scales"]):
            lat = g[f"{key}/latents"].to(DEV, copy=True)
            lat_in = torch.full((n,), float("nan"), device=DEV)
            eps = torch.full((n,), float("nan"), device=DEV)
            ops.sched_step(np_, counter, lat, None, lat_in, C_=C, F=F, HW=HW, guidance_scale=gs, a=p.a, b=p.b, c_x=p.c_x, c=p.c,
                           slot=(-1, -1, -1, -1), c_noise=p.c_noise, s_next=p.s_next, seed=int(meta["seed"]), step=si, eps_out=eps)
            torch.cuda.synchronize()
            assert torch.equal(lat.cpu(), g[f"{key}/gs{gs}/{name}/latents"]), (name, gs)
            assert torch.equal(eps.cpu(), g[f"{key}/gs{gs}/eps"]), (name, gs)
            assert torch.equal(lat_in, lat), (name, gs)          # s_next = 1: the next model input is x' itself


def test_sched_step_refuses_bad_slots():
    from emote_hack_amd import _lib, ops
    n = 4 * 2 * 8
    t = torch.zeros(2, n, device=DEV)
    with pytest.raises(_lib.EmoHipError):   # the slot written is one read
        ops.sched_step(t, torch.ones(2, device=DEV), torch.zeros(n, device=DEV), torch.zeros(4, n, device=DEV), None, C_=4, F=2, HW=8,
                       guidance_scale=7.5, a=0, b=1, c_x=1, c=(1, 1, 0, 0), slot=(1, 1, -1, -1), c_noise=0, s_next=1, seed=0, step=0)


def test_timestep_embedding_f32():
    """Integral values: the f32 entry gives the int64 entry's bits.  Fractional values: the oracle's embedding."""
    from emote_hack_amd import ops
    from oracle.unet_ref import timestep_embedding
    dim = 320
    half = dim // 2
    import math
    freqs = torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float32) / half).to(DEV)
    ti = torch.tensor([0, 1, 261, 500, 981, 999], dtype=torch.int64, device=DEV)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        a = ops.timestep_embedding(ti, freqs, dim, True, dtype)
        b = ops.timestep_embedding(ti.float(), freqs, dim, True, dtype)
        assert torch.equal(a, b), dtype
    tf = torch.tensor([978.6, 500.5, 0.25, 13.875], dtype=torch.float32)
    got = ops.timestep_embedding(tf.to(DEV), freqs, dim, True, torch.float32).cpu()
    want = timestep_embedding(tf, dim, flip_sin_to_cos=True, freq_shift=0)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=2e-5)
    assert not torch.equal(got, ops.timestep_embedding(tf.long().to(DEV), freqs, dim, True, torch.float32).cpu())
