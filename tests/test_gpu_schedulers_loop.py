"""The sigma-space samplers (DPM-Solver++ 2M, Euler, Euler-ancestral, LMS) through the HIP loop: against the oracle loop
(oracle.pipeline_ref.denoise_loop) driven by test-local, stateful float64 schedulers written in diffusers' step form (model-output
lists, exp(-h), quadrature) - not in the linear plan form the product uses; graph replay; clip re-use; skipped steps; the UNet at
a fractional timestep."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from emote_hack_amd.synth import seeded_randn, synth_state_dict
from tests import cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 6


def _build(cfg, dtype, prefix="", cls=None, has_out=True):
    from emote_hack_amd.unet import UNet3DConditionModel
    from emote_hack_amd.spec import param_shapes
    cls = cls or UNet3DConditionModel
    m = cls(**cfg) if has_out else cls(**cfg, _has_out=False)
    m.load_state_dict(synth_state_dict(param_shapes(m.spec), prefix=prefix))
    return m.to(DEV, dtype)


def _product(name, **kw):
    from emote_hack_amd import (DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler,
                                LMSDiscreteScheduler)
    cls = dict(dpm=DPMSolverMultistepScheduler, euler=EulerDiscreteScheduler, euler_a=EulerAncestralDiscreteScheduler,
               lms=LMSDiscreteScheduler)[name]
    return cls(beta_schedule="scaled_linear", steps_offset=1, **kw)   # (the offset the pipeline ctor forces anyway)


class OracleSched:
    """diffusers-form float64 step of the four samplers over the product's (separately pinned) tables.  `start`: the first step
    that runs - set_timesteps hands the oracle loop only the tail, the step index stays global (the noise key of Euler-a)."""
    eta = 0.0

    def __init__(self, name, start=0, **kw):
        self.name, self.start, self.tables = name, start, _product(name, **kw)
        self.kind = "ddpm" if name == "euler_a" else "ddim"     # the oracle draws counter_normal noise for "ddpm"
        self.cfg = self.tables.config

    def set_timesteps(self, n):
        self.all = self.tables.set_timesteps(n)
        self.sig = self.tables.sigmas.double()
        self.i, self.outs = self.start, []
        return self.all[self.start:]

    def scale_model_input(self, x, t):
        if self.name == "dpm":
            return x
        s = float(self.sig[self.all.index(t)])
        return x / math.sqrt(s * s + 1)

    def step(self, eps, t, x, noise=None):
        i = self.i
        self.i += 1
        assert self.all[i] == t
        x, eps = x.double(), eps.double()
        s, s1 = self.sig[i], self.sig[i + 1]
        if self.name == "euler":
            x0 = x - s * eps
            out = x + (x - x0) / s * (s1 - s)
        elif self.name == "euler_a":
            x0 = x - s * eps
            up = (s1 ** 2 * (s ** 2 - s1 ** 2) / s ** 2) ** 0.5
            down = (s1 ** 2 - up ** 2) ** 0.5
            out = x + (x - x0) / s * (down - s) + noise.double() * up
        elif self.name == "lms":
            self.outs.append((x - (x - s * eps)) / s)
            self.outs = self.outs[-4:]
            order = len(self.outs)
            nodes = [float(self.sig[i - k]) for k in range(order)]
            xg, wg = np.polynomial.legendre.leggauss(4)
            a, b = float(s), float(s1)
            tau = 0.5 * (b - a) * xg + 0.5 * (a + b)
            out = x
            for j in range(order):
                basis = np.ones_like(tau)
                for k in range(order):
                    if k != j:
                        basis = basis * (tau - nodes[k]) / (nodes[j] - nodes[k])
                out = out + 0.5 * (b - a) * float(np.dot(wg, basis)) * self.outs[-1 - j]
        else:   # DPM-Solver++ (midpoint), diffusers' multistep_dpm_solver_{first,second}_order_update
            def vp(v):
                v = torch.tensor(float(v), dtype=torch.float64)
                al = 1 / torch.sqrt(v * v + 1)
                return al, v * al
            a_s, sg_s = vp(s)
            a_t, sg_t = vp(s1)
            x0 = (x - sg_s * eps) / a_s
            self.outs.append(x0)
            lam_s, lam_t = torch.log(a_s) - torch.log(sg_s), torch.log(a_t) - torch.log(sg_t)
            h = lam_t - lam_s
            n = len(self.all)
            final = i == n - 1 and ((self.cfg.lower_order_final and n < 15) or self.cfg.final_sigmas_type == "zero")
            if len(self.outs) == 1 or final:
                out = (sg_t / sg_s) * x - (a_t * (torch.exp(-h) - 1.0)) * x0
            else:
                a_p, sg_p = vp(self.sig[i - 1])
                h0 = lam_s - (torch.log(a_p) - torch.log(sg_p))
                r0 = h0 / h
                D0, D1 = self.outs[-1], (self.outs[-1] - self.outs[-2]) / r0
                out = (sg_t / sg_s) * x - (a_t * (torch.exp(-h) - 1.0)) * D0 - 0.5 * (a_t * (torch.exp(-h) - 1.0)) * D1
        return out.float()


_MODELS = {}


def _models(dtype=torch.float32):
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    if dtype not in _MODELS:
        _MODELS[dtype] = (_build(cases.TINY, dtype, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False),
                          _build(cases.TINY_MOTION, dtype))
    return _MODELS[dtype]


def _inputs(init_sigma):
    return seeded_randn((1, 4, 8, 16, 16), 5) * init_sigma, seeded_randn((1, 4, 16, 16), 3), seeded_randn((2, 5, 32), 2)


KW = dict(guidance_scale=7.5, context_frames=4, context_stride=1, context_overlap=2, seed=0)
# The eps trace is held to the loop-golden tolerance (1e-3 / 1e-4).  The latents of a sigma-space sampler integrate eps over sigma
# from sigma_max (14.6 here) down to 0 - x' = x + (sigma_next - sigma) eps for Euler - so an eps difference within that tolerance
# reaches them multiplied by up to sigma_max: their absolute tolerance is 1e-4 * sigma_max.
LAT_ATOL = 1e-4 * 14.6


def _hip_loop(sch, lat, refl, text, dtype=torch.float32, pipe=None, **kw):
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    ref, unet = _models(dtype)
    pipe = pipe or EMOAnimationPipeline(unet=unet, scheduler=sch)
    args = dict(KW, num_inference_steps=STEPS, appearance_encoder=ref)
    args.update(kw)
    return pipe.denoise(lat.to(DEV), refl, text, **args), pipe


_ORACLE = {}


def _oracle(name, start=0, **skw):
    key = (name, start, tuple(sorted(skw.items())))
    if key not in _ORACLE:
        from oracle.pipeline_ref import denoise_loop
        from emote_hack_amd.spec import build_spec, param_shapes
        ref, _ = _models()
        usd = synth_state_dict(param_shapes(build_spec(cases.TINY_MOTION)))
        rsd = synth_state_dict(param_shapes(ref.spec), prefix=cases.REF_PREFIX)
        sch = OracleSched(name, start, **skw)
        sch.tables.set_timesteps(STEPS)
        lat, refl, text = _inputs(sch.tables.init_noise_sigma)
        _ORACLE[key] = denoise_loop(usd, cases.TINY_MOTION, rsd, cases.TINY, lat, refl, text, scheduler=sch,
                                    num_inference_steps=STEPS, return_eps=True, **KW)
    return _ORACLE[key]


@pytest.mark.parametrize("name,skw", [("dpm", {}), ("dpm", dict(use_karras_sigmas=True)), ("euler", {}), ("euler_a", {}),
                                      ("lms", {}), ("lms", dict(timestep_spacing="leading"))])
@pytest.mark.parametrize("graphs", [False, True])
def test_loop_against_oracle(name, skw, graphs):
    """8 frames in windows of 4 with overlap 2, CFG 7.5, the ReferenceNet, f32, 6 steps: eps trace and final latents at the
    loop-golden tolerance."""
    want_lat, want_eps = _oracle(name, **skw)
    sch = _product(name, **skw)
    sch.set_timesteps(STEPS)
    lat, refl, text = _inputs(sch.init_noise_sigma)
    (got_lat, got_eps), _ = _hip_loop(sch, lat, refl, text, return_eps=True, use_graphs=graphs)
    assert len(got_eps) == STEPS
    for i in range(STEPS):
        torch.testing.assert_close(got_eps[i].cpu(), want_eps[i], rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(got_lat.cpu(), want_lat, rtol=1e-3, atol=LAT_ATOL)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["euler", "dpm"])
def test_graph_replay_is_bit_identical(name, dtype):
    """A step-dependent input scale or a float timestep baked into a captured graph would move the latents."""
    outs = []
    for graphs in (False, True):
        sch = _product(name)
        sch.set_timesteps(STEPS)
        lat, refl, text = _inputs(sch.init_noise_sigma)
        out, _ = _hip_loop(sch, lat, refl, text, dtype=dtype, use_graphs=graphs, reference_group=2)
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("name", ["lms", "dpm", "euler_a"])
def test_clip_reuse_equals_a_fresh_pipeline(name):
    """A second clip on the kept state (history ring, lat_in, plan re-armed) equals a fresh pipeline's clip bit for bit.
    reference_group 4 of 6 steps: ReferenceNet groups of 4 and 2 timesteps, whose captured passes alternate on the kept state."""
    sch = _product(name)
    sch.set_timesteps(STEPS)
    lat, refl, text = _inputs(sch.init_noise_sigma)
    lat2 = seeded_randn((1, 4, 8, 16, 16), 9) * sch.init_noise_sigma
    _, pipe = _hip_loop(sch, lat, refl, text, reuse_state=True, use_graphs=True, reference_group=4)
    again, _ = _hip_loop(sch, lat2, refl, text, pipe=pipe, reuse_state=True, use_graphs=True, reference_group=4)
    fresh, _ = _hip_loop(_product(name), lat2, refl, text, use_graphs=True, reference_group=4)
    assert torch.equal(again.cpu(), fresh.cpu())


def test_skipped_steps_dpm_against_oracle():
    """num_actual_inference_steps = 4 of 6: the loop starts at step 2, with DPM-Solver++ at order 1 there."""
    start = 2
    want_lat, want_eps = _oracle("dpm", start=start)
    sch = _product("dpm")
    sch.set_timesteps(STEPS)
    lat, refl, text = _inputs(sch.init_noise_sigma)
    (got_lat, got_eps), _ = _hip_loop(sch, lat, refl, text, return_eps=True, num_actual_inference_steps=STEPS - start)
    assert len(got_eps) == STEPS - start
    for i in range(STEPS - start):
        torch.testing.assert_close(got_eps[i].cpu(), want_eps[i], rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(got_lat.cpu(), want_lat, rtol=1e-3, atol=LAT_ATOL)


def test_unet_fractional_timestep():
    """t = 500.5 reaches the embedding unrounded (Python float and float tensor), like the reference's time_proj."""
    from emote_hack_amd.spec import build_spec, param_shapes
    from oracle.unet_ref import unet_forward
    _, unet = _models()
    usd = synth_state_dict(param_shapes(build_spec(cases.TINY_MOTION)))
    x, ctx = cases.tiny_inputs(batch=1)
    want = unet_forward(usd, cases.TINY_MOTION, x, 500.5, ctx)
    got = unet(x.to(DEV), 500.5, ctx.to(DEV)).sample.cpu()
    torch.testing.assert_close(got, want, rtol=1e-3, atol=1e-4)
    got_t = unet(x.to(DEV), torch.tensor([500.5], device=DEV), ctx.to(DEV)).sample.cpu()
    assert torch.equal(got, got_t)
    at500 = unet(x.to(DEV), 500, ctx.to(DEV)).sample.cpu()
    assert not torch.equal(got, at500)
    assert torch.equal(unet(x.to(DEV), 500.0, ctx.to(DEV)).sample.cpu(), at500)   # integral float = the int64 path's bits

