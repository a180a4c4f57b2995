"""Schedulers of the sampling loop (call sites EMOAnimationPipeline.py:653-654,764,817): DDPM / DDIM, and the sigma-space
samplers below (DPM-Solver++ 2M, Euler, Euler-ancestral, LMS).

The reference uses `diffusers` schedulers (not in its tree, version unpinned) - restated here from
the papers (DDPM: Ho et al. 2020 Eq. 7/11, "fixed_small" variance; DDIM: Song et al. 2021 Eq. 12).
Every scheduler serves one protocol: per step the host computes, in float64, a PLAN `step_plan(si, first)` of the linear form
the fused HIP step kernel (emo_sched_step) evaluates per element, with counter-based noise, so every rank draws identical z
without communication:
  d_n   = a*x + b*eps                       (the solver's model output: eps, or x0 = (x - sigma_t*eps) / alpha_t)
  x'    = c_x*x + sum_k c[k]*d_{n-k} + c_noise*z   (k = 0..3; d_{n-k} from a ring of `history` earlier model outputs)
  x_in  = s_next*x'                         (scale_model_input of the NEXT step, `input_scale(si + 1)`)
A multistep warm-up counts from the first step that RUNS (`first`), so a loop started late begins at order 1.
DDPM / DDIM compute the INTEGER timestep table (bit-exact) and three scalars per step, `coefficients(t)`:
x' = c_x*x + c_eps*eps + c_noise*z, the plan a = 0, b = 1, c = (c_eps,), no ring, an unscaled model input.

Pipeline-enforced config (EMOAnimationPipeline.py:105-130): steps_offset=1 on every scheduler whose config carries the key
(both classes here do, like diffusers' since `timestep_spacing` exists), clip_sample=False.  A scheduler built on its own keeps
diffusers' defaults (DDIM: the pipeline's 1; DDPM: 0) until it is handed to EMOAnimationPipeline.
`timestep_spacing` is "leading" (diffusers' default for both classes: i * (T // n) + steps_offset); other spacings are refused.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch


class StepPlan(SimpleNamespace):
    """a, b, c_x, c (4 floats: d_n, d_{n-1}, d_{n-2}, d_{n-3}), c_noise, s_next - see the module docstring"""


class _PlanBase:
    """The step-plan protocol every scheduler of the loop serves.  Subclasses set `float_timesteps`, `history` (model-output
    ring slots the plan needs) and implement `_plan`; `input_scale` when the model input is scaled."""
    order = 1
    history = 0

    def input_scale(self, si):
        """scale_model_input factor of step si"""
        return 1.0

    def step_plan(self, si, first=0):
        """StepPlan of step si for a loop whose first executed step is `first` (the multistep warm-up counts from there)"""
        if not first <= si < len(self.timesteps):
            raise IndexError(f"step {si} outside [{first}, {len(self.timesteps)})")
        p = self._plan(si, first)
        p.c = tuple(float(v) for v in p.c) + (0.0,) * (4 - len(p.c))
        p.s_next = self.input_scale(si + 1) if si + 1 < len(self.timesteps) else 1.0
        return p


def _betas(T, beta_start, beta_end, schedule):
    if schedule == "linear":
        return torch.linspace(beta_start, beta_end, T, dtype=torch.float32)
    if schedule == "scaled_linear":
        return torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float32) ** 2
    raise NotImplementedError(f"{schedule} is not implemented")


class _SchedulerBase(_PlanBase):
    init_noise_sigma = 1.0
    float_timesteps = False

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear",
                 steps_offset=0, clip_sample=False, set_alpha_to_one=True, timestep_spacing="leading", **_ignored):
        if clip_sample:
            raise ValueError("clip_sample must be False (EMOAnimationPipeline.py:118-130 forces it)")
        if timestep_spacing != "leading":
            raise NotImplementedError(f"timestep_spacing={timestep_spacing!r}: only 'leading' (the diffusers default the reference runs) is built")
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, steps_offset=steps_offset, clip_sample=False,
                                      set_alpha_to_one=set_alpha_to_one, timestep_spacing=timestep_spacing)
        self.betas = _betas(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, dim=0).double()
        self.final_alpha_cumprod = 1.0 if set_alpha_to_one else float(self.alphas_cumprod[0])
        self.num_inference_steps = None
        self.timesteps = None

    def set_timesteps(self, num_inference_steps, device=None):
        T = self.config.num_train_timesteps
        if num_inference_steps > T:
            raise ValueError("num_inference_steps > num_train_timesteps")
        self.num_inference_steps = num_inference_steps
        ratio = T // num_inference_steps
        self.timesteps = [int(i * ratio) + self.config.steps_offset for i in range(num_inference_steps)][::-1]
        return self.timesteps

    def scale_model_input(self, sample, timestep=None):
        return sample

    def _alphas(self, t):
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = float(self.alphas_cumprod[t])
        a_prev = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else self._final_alpha()
        return a_t, a_prev

    def _plan(self, si, first):
        c_x, c_eps, c_n = self.coefficients(self.timesteps[si])
        return StepPlan(a=0.0, b=1.0, c_x=c_x, c=(c_eps,), c_noise=c_n)


class DDIMScheduler(_SchedulerBase):
    """steps_offset defaults to 1 (the pipeline forces it)."""

    def __init__(self, *a, steps_offset=1, eta=0.0, **kw):
        super().__init__(*a, steps_offset=steps_offset, **kw)
        self.eta = eta

    def _final_alpha(self):
        return self.final_alpha_cumprod

    def coefficients(self, t, eta=None):
        eta = self.eta if eta is None else eta
        a_t, a_prev = self._alphas(t)
        var = (1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)
        std = eta * math.sqrt(max(var, 0.0))
        c_x = math.sqrt(a_prev / a_t)
        c_eps = -math.sqrt(a_prev) * math.sqrt(1 - a_t) / math.sqrt(a_t) + math.sqrt(max(1 - a_prev - std * std, 0.0))
        return c_x, c_eps, std


class DDPMScheduler(_SchedulerBase):
    def _final_alpha(self):
        return 1.0

    def coefficients(self, t, eta=None):
        a_t, a_prev = self._alphas(t)
        cur_alpha = a_t / a_prev
        cur_beta = 1 - cur_alpha
        k0 = math.sqrt(a_prev) * cur_beta / (1 - a_t)       # coefficient of x0 (Eq. 7)
        kx = math.sqrt(cur_alpha) * (1 - a_prev) / (1 - a_t)  # coefficient of x_t
        c_x = k0 / math.sqrt(a_t) + kx
        c_eps = -k0 * math.sqrt(1 - a_t) / math.sqrt(a_t)
        c_n = math.sqrt(max((1 - a_prev) / (1 - a_t) * cur_beta, 1e-20)) if t > 0 else 0.0
        return c_x, c_eps, c_n


# ============================================================================ sigma-space samplers
# DPM-Solver++ (Lu et al. 2022, "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic Models", Alg. 2 / the
# multistep second-order "2M" update), Euler and Euler-ancestral (Karras et al. 2022, "Elucidating the Design Space of
# Diffusion-Based Generative Models", Alg. 1 with S_churn = 0 and the sigma_up / sigma_down split of its ancestral variant),
# and linear multistep (LMS, the k-diffusion sampler after Karras et al.'s sigma-space ODE dx/dsigma = eps).  Behaviour restated
# from the papers in the form diffusers ~0.26-0.27 (the release the reference's import sites imply) gives them: VP
# alphas_cumprod, sigma = sqrt((1 - alpha_bar) / alpha_bar), the same timestep spacings, init_noise_sigma and model-input scale.


def _spaced(T, n, spacing, steps_offset, plus_one=False):
    """float64 timestep grid of the three `timestep_spacing` modes, descending.  plus_one: DPM-Solver's variant (n + 1 points
    with the last one dropped for linspace / leading), Euler's / LMS' otherwise."""
    import numpy as np
    if spacing == "linspace":
        if plus_one:
            return np.linspace(0, T - 1, n + 1).round()[::-1][:-1].copy()
        return np.linspace(0, T - 1, n)[::-1].copy()
    if spacing == "leading":
        if plus_one:
            ratio = T // (n + 1)
            return (np.arange(0, n + 1) * ratio).round()[::-1][:-1].astype(np.float64) + steps_offset
        ratio = T // n
        return (np.arange(0, n) * ratio).round()[::-1].astype(np.float64) + steps_offset
    if spacing == "trailing":
        ratio = T / n
        return np.round(np.arange(T, 0, -ratio)) - 1
    raise ValueError(f"timestep_spacing={spacing!r}: 'linspace', 'leading' or 'trailing'")


def _karras(sigma_min, sigma_max, n, rho=7.0):
    """Karras et al. 2022 Eq. 5: sigma_i = (sigma_max^(1/rho) + i/(n-1) (sigma_min^(1/rho) - sigma_max^(1/rho)))^rho."""
    import numpy as np
    ramp = np.linspace(0, 1, n)
    lo, hi = sigma_min ** (1 / rho), sigma_max ** (1 / rho)
    return (hi + ramp * (lo - hi)) ** rho


def _sigma_to_t(sigma, log_sigmas):
    """fractional training timestep of sigma: linear interpolation in log-sigma (clamped to [0, T-1])"""
    import numpy as np
    return np.interp(np.log(np.maximum(sigma, 1e-10)), log_sigmas, np.arange(len(log_sigmas), dtype=np.float64))


class _SigmaSchedulerBase(_PlanBase):
    """Shared table handling of the sigma-space samplers (see the block comment above).  Subclasses implement `_tables`, and the
    plan protocol's `_plan`; input_scale is 1 (the VP-form DPM-Solver) unless overridden."""
    float_timesteps = True

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=0,
                 clip_sample=False, timestep_spacing="linspace", use_karras_sigmas=False, prediction_type="epsilon", **_ignored):
        if clip_sample:
            raise ValueError("clip_sample must be False (EMOAnimationPipeline.py:118-130 forces it)")
        if timestep_spacing not in ("linspace", "leading", "trailing"):
            raise ValueError(f"timestep_spacing={timestep_spacing!r}: 'linspace', 'leading' or 'trailing'")
        if prediction_type != "epsilon":
            raise NotImplementedError(f"prediction_type={prediction_type!r}: only 'epsilon' (the reference's UNet) is built")
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, steps_offset=steps_offset, clip_sample=False,
                                      timestep_spacing=timestep_spacing, use_karras_sigmas=bool(use_karras_sigmas),
                                      prediction_type=prediction_type)
        self.betas = _betas(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, dim=0).double()
        self.num_inference_steps = None
        self.timesteps = None
        self.sigmas = None

    def _train_sigmas(self):
        ac = self.alphas_cumprod.numpy()
        return ((1 - ac) / ac) ** 0.5

    def set_timesteps(self, num_inference_steps, device=None):
        T = self.config.num_train_timesteps
        if num_inference_steps > T:
            raise ValueError("num_inference_steps > num_train_timesteps")
        self.num_inference_steps = num_inference_steps
        ts, sig = self._tables(num_inference_steps)
        self.timesteps = [float(t) for t in ts] if self.float_timesteps else [int(t) for t in ts]
        self.sigmas = torch.tensor(sig, dtype=torch.float64)    # n + 1 entries, the last one the final sigma
        return self.timesteps

    def step_index(self, timestep):
        if self.timesteps is None:
            raise RuntimeError("set_timesteps first")
        t = float(timestep.reshape(-1)[0]) if torch.is_tensor(timestep) else float(timestep)
        return min(range(len(self.timesteps)), key=lambda i: abs(self.timesteps[i] - t))

    def scale_model_input(self, sample, timestep=None):
        if timestep is None:
            raise ValueError(f"{type(self).__name__}.scale_model_input needs the timestep: the scale depends on the step")
        return sample * self.input_scale(self.step_index(timestep))


class _KarrasSigmaScheduler(_SigmaSchedulerBase):
    """Euler / Euler-ancestral / LMS tables: sigmas interpolated at fractional timesteps, model input x / sqrt(sigma^2 + 1)."""

    def _tables(self, n):
        import numpy as np
        c = self.config
        ts = _spaced(c.num_train_timesteps, n, c.timestep_spacing, c.steps_offset)
        train = self._train_sigmas()
        sig = np.interp(ts, np.arange(len(train), dtype=np.float64), train)
        if c.use_karras_sigmas:   # range of the interpolated schedule, timesteps mapped back through log-sigma
            sig = _karras(sig[-1], sig[0], n)
            ts = _sigma_to_t(sig, np.log(train))
        return ts, np.concatenate([sig, [0.0]])

    @property
    def init_noise_sigma(self):
        """sigma_max for 'linspace' / 'trailing', sqrt(sigma_max^2 + 1) for 'leading' (diffusers' convention)"""
        m = float(self.sigmas.max())
        return m if self.config.timestep_spacing in ("linspace", "trailing") else (m * m + 1) ** 0.5

    def input_scale(self, si):
        s = float(self.sigmas[si])
        return 1.0 / math.sqrt(s * s + 1.0)


class EulerDiscreteScheduler(_KarrasSigmaScheduler):
    """Karras et al. 2022 Alg. 1 (Euler, S_churn = 0): x' = x + (sigma_next - sigma) * eps, eps = dx/dsigma of the
    probability-flow ODE.  Float timesteps."""

    def __init__(self, *a, s_churn=0.0, **kw):
        if s_churn:
            raise NotImplementedError("s_churn > 0 is not built (diffusers' default 0 is)")
        super().__init__(*a, **kw)

    def _plan(self, si, first):
        s, s1 = float(self.sigmas[si]), float(self.sigmas[si + 1])
        return StepPlan(a=0.0, b=1.0, c_x=1.0, c=(s1 - s,), c_noise=0.0)


class EulerAncestralDiscreteScheduler(_KarrasSigmaScheduler):
    """Euler-ancestral (k-diffusion `sample_euler_ancestral`, eta = 1): sigma_up = sqrt(s1^2 (s^2 - s1^2) / s^2),
    sigma_down = sqrt(s1^2 - sigma_up^2); x' = x + (sigma_down - sigma) * eps + sigma_up * z.  z is the project's
    counter-based N(0, 1) keyed by (seed, step, element), not a torch generator: identical on every rank.
    Karras sigmas are not offered (diffusers 0.26-0.27 has none for this class)."""

    def __init__(self, *a, use_karras_sigmas=False, **kw):
        if use_karras_sigmas:
            raise NotImplementedError("EulerAncestralDiscreteScheduler: use_karras_sigmas is not built")
        super().__init__(*a, **kw)

    def _plan(self, si, first):
        s, s1 = float(self.sigmas[si]), float(self.sigmas[si + 1])
        up = math.sqrt(max(s1 * s1 * (s * s - s1 * s1) / (s * s), 0.0))
        down = math.sqrt(max(s1 * s1 - up * up, 0.0))
        return StepPlan(a=0.0, b=1.0, c_x=1.0, c=(down - s,), c_noise=up)


class LMSDiscreteScheduler(_KarrasSigmaScheduler):
    """Linear multistep in sigma (k-diffusion `sample_lms`): x' = x + sum_j c_j eps_{n-j}, c_j = integral over
    [sigma_n, sigma_{n+1}] of the Lagrange basis polynomial of node sigma_{n-j} on the nodes sigma_n..sigma_{n-order+1}.
    The integrand is a polynomial: the integral is exact (numpy.polynomial), no quadrature.  Order 4 (`order`), warming up
    from order 1 at the first step that runs."""
    history = 4

    def __init__(self, *a, order=4, **kw):
        if not 1 <= order <= 4:
            raise ValueError("LMS order must be 1..4")
        super().__init__(*a, **kw)
        self.config.lms_order = self.lms_order = order

    def lms_coefficient(self, order, si, j):
        from numpy.polynomial import polynomial as P
        sig = self.sigmas.numpy()
        poly, den = [1.0], 1.0
        for k in range(order):
            if k != j:
                poly = P.polymul(poly, [-sig[si - k], 1.0])
                den *= sig[si - j] - sig[si - k]
        integ = P.polyint(poly)
        return float((P.polyval(sig[si + 1], integ) - P.polyval(sig[si], integ)) / den)

    def _plan(self, si, first):
        order = min(si - first + 1, self.lms_order)
        return StepPlan(a=0.0, b=1.0, c_x=1.0, c=tuple(self.lms_coefficient(order, si, j) for j in range(order)), c_noise=0.0)


class DPMSolverMultistepScheduler(_SigmaSchedulerBase):
    """DPM-Solver++ (Lu et al. 2022) in data prediction, multistep, solver_type 'midpoint'; order 1 (= DDIM in lambda) or 2
    ("2M").  With lambda = log(alpha_t / sigma_t), h = lambda_t - lambda_s, x0 = (x - sigma_s eps) / alpha_s:
      order 1: x_t = (sigma_t / sigma_s) x - alpha_t (e^-h - 1) x0_n
      order 2: D0 = x0_n, D1 = (x0_n - x0_{n-1}) / r, r = h_{n-1} / h;  x_t = (sigma_t / sigma_s) x - alpha_t (e^-h - 1) (D0 + D1 / 2)
    (alpha_t, sigma_t are the VP pair 1 / sqrt(1 + s^2), s / sqrt(1 + s^2) of the k-diffusion sigma s).  Integer timesteps; the
    model input is not scaled; init_noise_sigma = 1.
    Version-dependent defaults, all constructor arguments: solver_order=2, lower_order_final=True (first order on the last step
    when fewer than 15 steps), final_sigmas_type='zero' (the last step lands on sigma = 0 and is then always first order;
    'sigma_min' ends at the smallest training sigma), use_karras_sigmas=False (True: Karras et al. Eq. 5 over the whole training
    range, timesteps rounded from log-sigma), timestep_spacing='linspace' (n + 1 points, the last dropped)."""
    float_timesteps = False
    history = 2

    def __init__(self, *a, solver_order=2, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
                 final_sigmas_type="zero", **kw):
        if algorithm_type != "dpmsolver++":
            raise NotImplementedError(f"algorithm_type={algorithm_type!r}: only 'dpmsolver++' is built")
        if solver_type != "midpoint":
            raise NotImplementedError(f"solver_type={solver_type!r}: only 'midpoint' is built")
        if solver_order not in (1, 2):
            raise NotImplementedError(f"solver_order={solver_order}: 1 or 2")
        if final_sigmas_type not in ("zero", "sigma_min"):
            raise ValueError(f"final_sigmas_type={final_sigmas_type!r}: 'zero' or 'sigma_min'")
        super().__init__(*a, **kw)
        self.config.solver_order, self.config.lower_order_final = solver_order, bool(lower_order_final)
        self.config.final_sigmas_type = final_sigmas_type
        self.config.algorithm_type, self.config.solver_type = algorithm_type, solver_type
        self.order = solver_order

    init_noise_sigma = 1.0

    def _tables(self, n):
        import numpy as np
        c = self.config
        ts = _spaced(c.num_train_timesteps, n, c.timestep_spacing, c.steps_offset, plus_one=True)
        train = self._train_sigmas()
        if c.use_karras_sigmas:
            sig = _karras(train[0], train[-1], n)
            ts = _sigma_to_t(sig, np.log(train)).round()
        else:
            sig = np.interp(ts, np.arange(len(train), dtype=np.float64), train)
        last = train[0] if c.final_sigmas_type == "sigma_min" else 0.0
        return ts, np.concatenate([sig, [last]])

    @staticmethod
    def _vp(s):
        a = 1.0 / math.sqrt(s * s + 1.0)
        return a, s * a     # alpha_t, sigma_t

    def _plan(self, si, first):
        c = self.config
        a_s, s_s = self._vp(float(self.sigmas[si]))
        a_t, s_t = self._vp(float(self.sigmas[si + 1]))
        # alpha_t (e^-h - 1) with e^-h = (alpha_s sigma_t) / (sigma_s alpha_t): finite at sigma_t = 0
        k = a_s * s_t / s_s - a_t
        n = len(self.timesteps)
        final = si == n - 1 and ((c.lower_order_final and n < 15) or c.final_sigmas_type == "zero")
        first_order = c.solver_order == 1 or si == first or final
        d = (1.0 / a_s, -s_s / a_s)            # x0 = (x - sigma_s eps) / alpha_s
        if first_order:
            return StepPlan(a=d[0], b=d[1], c_x=s_t / s_s, c=(-k,), c_noise=0.0)
        if s_t == s_s:   # (Karras sigmas ending on sigma_min, final_sigmas_type 'sigma_min': a zero-length last step)
            return StepPlan(a=d[0], b=d[1], c_x=1.0, c=(0.0,), c_noise=0.0)
        a_p, s_p = self._vp(float(self.sigmas[si - 1]))
        lam = lambda a_, s_: math.log(a_) - math.log(s_)
        h = lam(a_t, s_t) - lam(a_s, s_s)
        r = (lam(a_s, s_s) - lam(a_p, s_p)) / h
        return StepPlan(a=d[0], b=d[1], c_x=s_t / s_s, c=(-k * (1.0 + 0.5 / r), k * 0.5 / r), c_noise=0.0)
