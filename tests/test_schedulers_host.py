"""Host side of the sigma-space samplers (DPMSolverMultistepScheduler, EulerDiscreteScheduler, EulerAncestralDiscreteScheduler,
LMSDiscreteScheduler): timestep / sigma tables against a float64 numpy restatement written here, and the per-step plans driven
through a numpy interpreter of the kernel's linear form against the closed-form probability-flow ODE of Gaussian data.  CPU only."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from emote_hack_amd import (DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler,
                            LMSDiscreteScheduler)

T = 1000
SPACINGS = ["linspace", "leading", "trailing"]
KARRAS_CLASSES = [EulerDiscreteScheduler, LMSDiscreteScheduler, DPMSolverMultistepScheduler]


def train_sigmas(beta_schedule="scaled_linear", b0=0.00085, b1=0.012):
    # the training schedule in f32, as the models were trained; everything after it in float64
    if beta_schedule == "linear":
        betas = torch.linspace(b0, b1, T, dtype=torch.float32)
    else:
        betas = torch.linspace(b0 ** 0.5, b1 ** 0.5, T, dtype=torch.float32) ** 2
    ac = torch.cumprod(1.0 - betas, 0).double().numpy()
    return np.sqrt((1.0 - ac) / ac)


def interp_sigma(t, sig):
    lo = np.floor(t).astype(np.int64).clip(0, T - 1)
    hi = (lo + 1).clip(max=T - 1)
    w = t - lo
    return (1 - w) * sig[lo] + w * sig[hi]


def karras(lo, hi, n, rho=7.0):
    return np.array([(hi ** (1 / rho) + i / (n - 1) * (lo ** (1 / rho) - hi ** (1 / rho))) ** rho for i in range(n)])


def sigma_to_t(s, sig):
    ls, out = np.log(sig), []
    for v in np.log(s):
        k = min(max(int(np.searchsorted(ls, v, side="right")) - 1, 0), T - 2)
        w = min(max((v - ls[k]) / (ls[k + 1] - ls[k]), 0.0), 1.0)
        out.append(k + w)
    return np.array(out)


def want_tables(cls, n, spacing, use_karras, offset=0):
    sig = train_sigmas()
    if cls is DPMSolverMultistepScheduler:   # n + 1 grid points, the last dropped; integer timesteps
        if spacing == "linspace":
            ts = np.array([round(999 * i / n) for i in range(n, 0, -1)], dtype=np.float64)
        elif spacing == "leading":
            ts = np.array([i * (T // (n + 1)) + offset for i in range(n, 0, -1)], dtype=np.float64)
        else:
            ts = np.array([round(T - i * T / n) - 1 for i in range(n)], dtype=np.float64)
        if use_karras:
            s = karras(sig[0], sig[-1], n)
            ts = np.round(sigma_to_t(s, sig))
        else:
            s = interp_sigma(ts, sig)
        return [int(t) for t in ts], np.append(s, 0.0)
    if spacing == "linspace":
        ts = np.array([999 * i / (n - 1) for i in range(n - 1, -1, -1)])
    elif spacing == "leading":
        ts = np.array([i * (T // n) + offset for i in range(n - 1, -1, -1)], dtype=np.float64)
    else:
        ts = np.array([round(T - i * T / n) - 1 for i in range(n)], dtype=np.float64)
    s = interp_sigma(ts, sig)
    if use_karras:
        s = karras(s[-1], s[0], n)
        ts = sigma_to_t(s, sig)
    return list(ts), np.append(s, 0.0)


@pytest.mark.parametrize("n", [10, 20, 25, 50])
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("use_karras", [False, True])
@pytest.mark.parametrize("cls", KARRAS_CLASSES + [EulerAncestralDiscreteScheduler])
def test_tables(cls, n, spacing, use_karras):
    if cls is EulerAncestralDiscreteScheduler and use_karras:
        with pytest.raises(NotImplementedError):
            cls(use_karras_sigmas=True)
        return
    sch = cls(beta_schedule="scaled_linear", timestep_spacing=spacing, use_karras_sigmas=use_karras, steps_offset=1)
    got = sch.set_timesteps(n)
    ts, sig = want_tables(cls, n, spacing, use_karras, offset=1)
    assert len(got) == n and sch.sigmas.shape == (n + 1,)
    if cls is DPMSolverMultistepScheduler:
        assert all(isinstance(t, int) for t in got) and got == ts           # integer table: bit-exact
        assert sch.init_noise_sigma == 1.0
    else:
        assert all(isinstance(t, float) for t in got)
        np.testing.assert_allclose(got, ts, rtol=1e-12, atol=1e-9)
        smax = float(sig.max())
        want_init = smax if spacing in ("linspace", "trailing") else math.sqrt(smax * smax + 1)
        assert sch.init_noise_sigma == pytest.approx(want_init, rel=1e-12)
        x = torch.ones(3, dtype=torch.float64)
        for si in (0, n // 2, n - 1):   # scale_model_input = x / sqrt(sigma^2 + 1), found by timestep
            assert float(sch.scale_model_input(x, got[si])[0]) == pytest.approx(1 / math.sqrt(sig[si] ** 2 + 1), rel=1e-12)
    np.testing.assert_allclose(sch.sigmas.numpy(), sig, rtol=1e-12, atol=1e-12)


def test_dpm_final_sigma_and_refusals():
    sig = train_sigmas()
    sch = DPMSolverMultistepScheduler(beta_schedule="scaled_linear", final_sigmas_type="sigma_min")
    sch.set_timesteps(20)
    assert float(sch.sigmas[-1]) == pytest.approx(sig[0], rel=1e-12)
    for bad in (dict(algorithm_type="dpmsolver"), dict(solver_type="heun"), dict(solver_order=3), dict(final_sigmas_type="x")):
        with pytest.raises((NotImplementedError, ValueError)):
            DPMSolverMultistepScheduler(**bad)
    with pytest.raises(ValueError):
        EulerDiscreteScheduler(timestep_spacing="bogus")
    with pytest.raises(NotImplementedError):                         # the existing classes keep refusing other spacings
        DDIMScheduler(timestep_spacing="linspace")


def test_lms_coefficients_against_gauss_legendre():
    """Exact polynomial integration against Gauss-Legendre quadrature (exact for the degree <= 3 Lagrange basis)."""
    sch = LMSDiscreteScheduler(beta_schedule="scaled_linear")
    sch.set_timesteps(12)
    s = sch.sigmas.numpy()
    xg, wg = np.polynomial.legendre.leggauss(4)
    for si in range(3, 11):
        a, b = s[si], s[si + 1]
        tau = 0.5 * (b - a) * xg + 0.5 * (a + b)
        for j in range(4):
            basis = np.prod([(tau - s[si - k]) / (s[si - j] - s[si - k]) for k in range(4) if k != j], axis=0)
            want = 0.5 * (b - a) * float(np.dot(wg, basis))
            assert sch.lms_coefficient(4, si, j) == pytest.approx(want, rel=1e-10, abs=1e-14)


def test_warmup_counts_from_first_step_that_runs():
    lms = LMSDiscreteScheduler()
    lms.set_timesteps(20)
    assert [sum(c != 0 for c in lms.step_plan(si, first=8).c) for si in range(8, 13)] == [1, 2, 3, 4, 4]
    dpm = DPMSolverMultistepScheduler()
    dpm.set_timesteps(20)
    assert dpm.step_plan(8, first=8).c[1] == 0.0 and dpm.step_plan(9, first=8).c[1] != 0.0
    assert dpm.step_plan(19, first=0).c[1] == 0.0       # final_sigmas_type="zero": the last step is first order
    dpm2 = DPMSolverMultistepScheduler(final_sigmas_type="sigma_min", lower_order_final=True)
    dpm2.set_timesteps(10)
    assert dpm2.step_plan(9).c[1] == 0.0                # lower_order_final below 15 steps
    dpm2.set_timesteps(20)
    assert dpm2.step_plan(19).c[1] != 0.0


# ---------------------------------------------------------------- analytic convergence
# Data x0 ~ N(0, S^2).  In sigma space (x = x0 + sigma * n) the exact eps-predictor is eps = sigma x / (S^2 + sigma^2) and the
# probability-flow ODE keeps x / sqrt(S^2 + sigma^2) constant.  The VP sample of DPM-Solver / DDIM is alpha * x, alpha = 1 /
# sqrt(1 + sigma^2).  The plans are driven through the kernel's linear form:
#   d_n = a x + b eps;  x' = c_x x + sum_k c_k d_{n-k} + c_noise z
S = 0.5


def eps_sigma(x, sigma):
    return sigma * x / (S * S + sigma * sigma)


def eps_vp(x, sigma):
    return eps_sigma(x * math.sqrt(1 + sigma * sigma), sigma)


def interpret(sch, n, x, steps, eps_fn, noise=None):
    hist = []
    for si in range(steps):
        p = sch.step_plan(si)
        sig = float(sch.sigmas[si])
        eps = eps_fn(x, sig)
        hist.insert(0, p.a * x + p.b * eps)
        x = p.c_x * x + sum(c * d for c, d in zip(p.c, hist))
        if p.c_noise:
            x = x + p.c_noise * noise(si)
        del hist[4:]
    return x


def ode_error(make, n, vp):
    """endpoint error of a unit start against the closed form, at the last nonzero sigma: the tables always end on t = 0 (or
    close to it) and the final jump into sigma = 0 (sigma_min) has a size that barely shrinks with n, which would floor the error
    of every solver alike - it is covered by the tables and the loop tests instead."""
    sch = make()
    sch.set_timesteps(n)
    sig = sch.sigmas.numpy()
    steps = n - 1
    s0, s1 = sig[0], sig[steps]
    x0 = 1.0 / math.sqrt(1 + s0 * s0) if vp else 1.0
    want = math.sqrt(S * S + s1 * s1) / math.sqrt(S * S + s0 * s0)
    if vp:
        want /= math.sqrt(1 + s1 * s1)
    got = interpret(sch, n, x0, steps, eps_vp if vp else eps_sigma)
    return abs(got - want)


def ddim_error(n):
    sch = DDIMScheduler(beta_schedule="scaled_linear")
    ts = sch.set_timesteps(n)
    ac = sch.alphas_cumprod.numpy()
    sig = lambda t: math.sqrt((1 - ac[t]) / ac[t])
    x = 1.0 / math.sqrt(1 + sig(ts[0]) ** 2)
    for t in ts[:-1]:
        c_x, c_eps, _ = sch.coefficients(t, 0.0)
        x = c_x * x + c_eps * eps_vp(x, sig(t))
    s0, s1 = sig(ts[0]), sig(ts[-1])
    want = math.sqrt(S * S + s1 * s1) / math.sqrt(S * S + s0 * s0) / math.sqrt(1 + s1 * s1)
    return abs(x - want)


CASES = {   # name -> (error(n), minimum observed order over both doublings)
    "euler": (lambda n: ode_error(lambda: EulerDiscreteScheduler(beta_schedule="scaled_linear"), n, False), 0.8),
    "euler_karras": (lambda n: ode_error(lambda: EulerDiscreteScheduler(beta_schedule="scaled_linear", use_karras_sigmas=True), n, False), 0.8),
    "lms": (lambda n: ode_error(lambda: LMSDiscreteScheduler(beta_schedule="scaled_linear"), n, False), 1.8),
    "lms_karras": (lambda n: ode_error(lambda: LMSDiscreteScheduler(beta_schedule="scaled_linear", use_karras_sigmas=True), n, False), 1.8),
    # DPM-Solver++ steps in lambda = log(alpha / sigma): a grid uniform in t crowds lambda's whole tail into a few steps of fixed size
    # near t = 0 (h -> 0.5 log 2 however large n is), so its order shows on the Karras grid, which refines every step
    "dpmpp_2m_karras": (lambda n: ode_error(lambda: DPMSolverMultistepScheduler(beta_schedule="scaled_linear", use_karras_sigmas=True),
                                            n, True), 1.8),
    "dpmpp_1_karras": (lambda n: ode_error(lambda: DPMSolverMultistepScheduler(beta_schedule="scaled_linear", solver_order=1,
                                                                               use_karras_sigmas=True), n, True), 0.8),
    "ddim_sanity": (ddim_error, 0.8),
}


@pytest.mark.parametrize("name", list(CASES))
def test_convergence_order(name):
    """The error shrinks at every doubling of n (10 -> 20 -> 40), and its observed order over the two doublings,
    log2(e10 / e40) / 2, is at least 0.8 for the first-order solvers (Euler, DPM-Solver++ 1, DDIM) and 1.8 for DPM-Solver++ 2M
    and LMS (a single doubling can land on a sign change of the error and overshoot, so the order is taken over both)."""
    err, min_order = CASES[name]
    e = [err(n) for n in (10, 20, 40)]
    assert e[0] > e[1] > e[2], (name, e)
    assert math.log2(e[0] / e[2]) / 2 >= min_order, (name, e)


def test_euler_ancestral_reaches_the_data_std():
    """With the exact predictor, Euler-ancestral samples of N(0, S^2) end with a std that approaches S as n grows.  The noise is the kernel's counter-based z (oracle.scheduler_ref.counter_normal)."""
    from oracle.scheduler_ref import counter_normal
    N = 200_000
    dev = []
    for n in (10, 20, 40):
        sch = EulerAncestralDiscreteScheduler(beta_schedule="scaled_linear")
        sch.set_timesteps(n)
        x = counter_normal(123, 10_000, N).double().numpy() * sch.init_noise_sigma
        x = interpret(sch, n, x, n, eps_sigma, noise=lambda si: counter_normal(7, si, N).double().numpy())
        dev.append(abs(float(x.std()) - S) / S)
    # ancestral sampling is weakly first order here: the std deficit roughly halves with every doubling of n
    assert dev[1] < 0.75 * dev[0] and dev[2] < 0.75 * dev[1], dev
    assert dev[2] < 0.15, dev


def test_unserved_scheduler_is_refused():
    from emote_hack_amd.pipeline import EMOAnimationPipeline

    class PNDMScheduler:
        config = type("C", (), {})()

    class CoefficientsOnlyScheduler:   # the DDIM / DDPM `coefficients(t, eta)` without the step-plan protocol
        config = type("C", (), {})()

        def coefficients(self, t, eta=None):
            return 1.0, 0.0, 0.0
    for sch in (PNDMScheduler(), CoefficientsOnlyScheduler()):
        with pytest.raises(TypeError, match=f"{type(sch).__name__} is not served"):
            EMOAnimationPipeline(unet=type("U", (), {"device": "cpu"})(), scheduler=sch)
