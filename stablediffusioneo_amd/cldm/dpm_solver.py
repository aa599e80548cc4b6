"""DPM-Solver++(2M) (Lu et al. 2022) with the surface of `DDIMSampler`: a deterministic second-order multistep solver of the
probability-flow ODE in the data-prediction form, on a grid uniform in log-SNR (or on DDIM's uniform-t grid).

With alpha = sqrt(a), sigma = sqrt(1 - a), lambda = ln(alpha / sigma), a step from a_t to a_next has h = lambda_next - lambda_t > 0,
phi = -expm1(-h), and D the CFG-combined data prediction (the pred_x0 of the DDIM kernels):

    first order   x_next = (sigma_next / sigma_t) x + alpha_next phi D                       (the eta = 0 DDIM step)
    second order  x_next = (sigma_next / sigma_t) x + alpha_next phi [(1 + 1/(2r)) D - (1/(2r)) D_prev],   r = h_prev / h

The host folds all of it into three fp64 coefficients per step, x_next = k_x x + k_d D + k_p D_prev; the device side
(`sdeo_cfg_dpmpp_2m_step`, `sdeo_dpmpp_2m_step`) never sees lambda.  The only state next to the latent is one fp32 tensor, D_prev.

The loop is DDIM's (`ddim_hacked.captured_loop`): step 1 runs eagerly (it fills the runtime's hint / context caches), steps 2..S are
replayed from a captured graph with the per-step coefficients baked in (with a mask: the masked steps, `ddim_hacked.mask_operands`); what
does not qualify (callbacks, a replaced q_sample, no ControlNet hint on one half, a model without a runtime) runs one step at a time; without
guidance (scale == 1 or no unconditional conditioning) the captured steps are the un-paired ones (SDEO_STEP_UNGUIDED).  The switches are ddim_hacked's (SDEO_GRAPH,
SDEO_LOOP_GRAPH, SDEO_LOOP_GRAPH_STEPS).

`DPMSolverSDESampler` is the stochastic member of the family, DPM-Solver++(2M) SDE (the same paper's SDE form; eta scales the injected
noise, eta = 1 is its 2M midpoint solver, eta = 0 the solver above).  It is the same linear update with one more term,

    x_next = (sigma_next / sigma_t) exp(-eta h) x + alpha_next (-expm1(-(1 + eta) h)) [(1 + 1/(2r)) D - (1/(2r)) D_prev]
             + sigma_next sqrt(-expm1(-2 eta h)) noise,          noise ~ N(0, I) drawn per step

which the host folds into four coefficients, x_next = k_x x + k_d D + k_p D_prev + k_n noise (`sde_coefficients`; the device side is
`sdeo_cfg_dpmpp_2m_sde_step` / `sdeo_dpmpp_2m_sde_step`).  Its first-order step at eta = 1 is the eta = 1 DDIM step.  The captured loop reads
each step's noise from a fixed row filled per image with the per-step loop's draws in its order (`ddim_hacked.draw_rows`), so a seed gives
the same latent on both paths.  Its grid defaults to log-SNR, and for a reason: on DDIM's uniform-t grid the last steps span most of the
log-SNR range (r = h_prev / h far below 1), the second-order weights 1 + 1/(2r) and -1/(2r) grow large, and the injected noise is
amplified through them -- on the Gaussian test problem (data variance 0.25, 10 steps, eta = 1) the final variance comes out 109 % too
large on the uniform grid against 2 to 8 % on the log-SNR grid (tests/test_stochastic_cpu.py).  At low step counts use it on `logsnr` only."""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from . import ddim_hacked as dh
from .ddim_hacked import DDIMSampler, make_ddim_timesteps

_DETERMINISTIC = "DPM-Solver++(2M) is a deterministic ODE solver: {} is not available (use DDIMSampler)"


def log_snr(alphas_cumprod):
    """lambda = ln(alpha / sigma) = (ln a - ln(1 - a)) / 2, fp64"""
    a = np.asarray(alphas_cumprod, dtype=np.float64)
    return 0.5 * (np.log(a) - np.log1p(-a))


def make_logsnr_timesteps(alphas_cumprod, S):
    """The S timesteps (decreasing, from T - 1) at which an S-step solver on a grid uniform in log-SNR evaluates the model: S + 1 points
    uniform in lambda from lambda(a[T-1]) to lambda(a[0]), each rounded to the integer timestep with the nearest lambda; where rounding
    collides (towards t = 0, where lambda moves fastest) the earlier point is pushed one timestep up.  The point after the last entry is
    t = 0: the last step lands on a[0], as DDIM's alphas_prev[0] does."""
    lam = log_snr(alphas_cumprod)
    T = lam.shape[0]
    if not 1 <= S < T:
        raise ValueError(f"{S} steps on a schedule of {T} timesteps")
    tau = [int(np.argmin(np.abs(lam - target))) for target in np.linspace(lam[T - 1], lam[0], S + 1)]
    for k in range(S, 0, -1):
        tau[k - 1] = max(tau[k - 1], tau[k] + 1)
    if tau[0] != T - 1:
        raise ValueError(f"{S} steps do not fit this schedule without leaving it (first timestep {tau[0]})")
    return np.asarray(tau[:S], dtype=np.int64)


def multistep_coefficients(alphas, alphas_next, lower_order_final=True):
    """(k_x, k_d, k_p) fp64 arrays of a run of steps a_t -> a_next that starts without history: the first step is first order, the last
    one too when lower_order_final (and there is more than one step)."""
    a_t, a_n = np.asarray(alphas, dtype=np.float64), np.asarray(alphas_next, dtype=np.float64)
    h = log_snr(a_n) - log_snr(a_t)
    assert (h > 0).all(), "every step must lower the noise level"
    phi = -np.expm1(-h)
    k_x = np.sqrt((1.0 - a_n) / (1.0 - a_t))
    k_d = np.sqrt(a_n) * phi
    k_p = np.zeros_like(k_d)
    n = h.shape[0]
    for k in range(1, n):
        if lower_order_final and k == n - 1:
            continue
        inv_2r = h[k] / (2.0 * h[k - 1])          # 1 / (2r), r = h_prev / h
        k_p[k] = -k_d[k] * inv_2r
        k_d[k] = k_d[k] * (1.0 + inv_2r)
    return k_x, k_d, k_p


def sde_coefficients(alphas, alphas_next, eta, lower_order_final=True):
    """(k_x, k_d, k_p, k_n) fp64 arrays of the DPM-Solver++(2M) SDE run of steps a_t -> a_next (symbols as in the module's docstring):
        k_x = (sigma_next / sigma_t) exp(-eta h),   w = alpha_next * -expm1(-(1 + eta) h),
        k_d = w (1 + 1/(2r)),  k_p = -w / (2r)  (first order: k_d = w, k_p = 0),   k_n = sigma_next sqrt(-expm1(-2 eta h))
    with the order rule of `multistep_coefficients`.  eta = 0 returns its three arrays bit for bit, and k_n = 0."""
    a_t, a_n = np.asarray(alphas, dtype=np.float64), np.asarray(alphas_next, dtype=np.float64)
    eta = float(eta)
    h = log_snr(a_n) - log_snr(a_t)
    assert (h > 0).all(), "every step must lower the noise level"
    k_x = np.sqrt((1.0 - a_n) / (1.0 - a_t)) * np.exp(-eta * h)
    k_d = np.sqrt(a_n) * -np.expm1(-((1.0 + eta) * h))
    k_p = np.zeros_like(k_d)
    k_n = np.sqrt(1.0 - a_n) * np.sqrt(-np.expm1(-2.0 * eta * h))
    n = h.shape[0]
    for k in range(1, n):
        if lower_order_final and k == n - 1:
            continue
        inv_2r = h[k] / (2.0 * h[k - 1])          # 1 / (2r), r = h_prev / h
        k_p[k] = -k_d[k] * inv_2r
        k_d[k] = k_d[k] * (1.0 + inv_2r)
    return k_x, k_d, k_p, k_n


class DPMSolverSampler(object):
    def __init__(self, model, discretize="logsnr", lower_order_final=True, **kwargs):
        super().__init__()
        if discretize not in ("logsnr", "uniform"):
            raise NotImplementedError(f'There is no discretization method called "{discretize}" (logsnr, uniform)')
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.discretize = discretize
        self.lower_order_final = bool(lower_order_final)
        self._pair = DDIMSampler(model)        # the fused cond / uncond forward and its conditioning cache are DDIM's (_eps_pair)
        self._schedule_key = None
        self._loop_key = None
        self.k_n = None                        # the noise coefficients of the stochastic subclass; None here: no step draws or adds noise

    # ------------------------------------------------------------------------------------------ schedule
    def make_schedule(self, ddim_num_steps, ddim_eta=0., verbose=True):
        """Host fp64 arrays, one entry per step in the order the loop takes them: timesteps (decreasing), alphas (a_t), alphas_next,
        k_x / k_d / k_p.  Cached like `DDIMSampler.make_schedule`, by the arguments and the identity of the model's schedule."""
        if ddim_eta != 0.:
            raise NotImplementedError(_DETERMINISTIC.format(f"eta = {ddim_eta}"))
        ac = self.model.alphas_cumprod
        fp = (id(ac), int(getattr(ac, "_version", 0)), int(ac.data_ptr()) if isinstance(ac, torch.Tensor) else 0, tuple(ac.shape))
        key = (int(ddim_num_steps), self.discretize, self.lower_order_final, id(self.model), self.ddpm_num_timesteps, fp)
        if self._schedule_key == key:
            return
        self._schedule_key = None
        acn = ac.detach().double().cpu().numpy() if isinstance(ac, torch.Tensor) else np.asarray(ac, dtype=np.float64)
        assert acn.shape[0] == self.ddpm_num_timesteps, "alphas have to be defined for each timestep"
        if self.discretize == "logsnr":
            ts = make_logsnr_timesteps(acn, int(ddim_num_steps))
        else:
            ts = np.flip(make_ddim_timesteps("uniform", int(ddim_num_steps), self.ddpm_num_timesteps, verbose=False)).astype(np.int64)
        if verbose:
            print(f"Selected timesteps for the DPM-Solver++(2M) sampler ({self.discretize}): {ts}")
        self.timesteps = ts
        self.alphas = acn[ts]
        self.alphas_next = np.append(acn[ts[1:]], acn[0])
        self.k_x, self.k_d, self.k_p, self.k_n = self._coefficients(self.alphas, self.alphas_next)
        self._schedule_key = key

    def _coefficients(self, alphas, alphas_next):
        """(k_x, k_d, k_p, k_n) of a run without history; k_n is None: the solver is deterministic"""
        return (*multistep_coefficients(alphas, alphas_next, self.lower_order_final), None)

    # ------------------------------------------------------------------------------------------ sample
    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, dynamic_threshold=None, ucg_schedule=None, **kwargs):
        """Signature and return value (samples, intermediates) of `DDIMSampler.sample`; intermediates["pred_x0"] holds D."""
        if eta != 0.:
            raise NotImplementedError(_DETERMINISTIC.format(f"eta = {eta}"))
        for name, off in (("score_corrector", score_corrector is None), ("quantize_x0", not quantize_x0),
                          ("dynamic_threshold", dynamic_threshold is None)):
            if not off:
                raise NotImplementedError(_DETERMINISTIC.format(name))
        if self.model.parameterization not in ("eps", "v"):
            raise NotImplementedError(f"parameterization {self.model.parameterization!r}: only eps and v are built")
        self.make_schedule(S, verbose=verbose)
        C, H, W = shape
        device = self.model.device
        size = (batch_size, C, H, W)
        img = torch.randn(size, device=device) if x_T is None else x_T.to(device=device, dtype=torch.float32)
        intermediates = {"x_inter": [img], "pred_x0": [img]}
        c, uc, scale = conditioning, unconditional_conditioning, unconditional_guidance_scale
        self._pair._cache_key = None
        total_steps = int(self.timesteps.shape[0])
        if (callback is None and img_callback is None and ucg_schedule is None and (mask is None or dh.mask_graph_ok(self.model, img, mask, x0))
                and (self.k_n is None or (temperature == 1. and noise_dropout == 0.))
                and self._loop_graph_ok(img, c, uc, scale, total_steps)):
            return self._loop_graphed(img, c, uc, scale, total_steps, log_every_t, intermediates, mask=mask, x0=x0)
        if mask is not None:
            assert x0 is not None
        x = self._run(img, c, uc, scale, self.timesteps, self.alphas, self.k_x, self.k_d, self.k_p, mask=mask, x0=x0, callback=callback,
                      img_callback=img_callback, ucg_schedule=ucg_schedule, log_every_t=log_every_t, intermediates=intermediates,
                      k_n=self.k_n, temperature=temperature, noise_dropout=noise_dropout,
                      plan=dh.control_plan(self._pair, c, uc, scale, total_steps))
        return x, intermediates

    def _step(self, x, d, c, uc, scale, k, timesteps, alphas, k_x, k_d, k_p, k_n=None, temperature=1., noise_dropout=0.):
        """one eager step: the model on the pair, then the update kernel; d (fixed buffer) holds D_prev on entry and D on return.
        With a noise coefficient (k_n[k] != 0, the stochastic subclass) the step draws torch.randn(x.shape, device=x.device) once, as
        `DDIMSampler.p_sample_ddim` does, temperature and noise_dropout meaning what they mean there."""
        ts = torch.full((x.shape[0],), int(timesteps[k]), device=x.device, dtype=torch.long)
        m_c, m_u = self._pair._eps_pair(x, c, ts, uc, scale)
        a_t = float(alphas[k])
        if k_n is not None and float(k_n[k]) != 0.:
            noise = torch.randn(x.shape, device=x.device).expand(x.shape).contiguous() * temperature
            if noise_dropout > 0.:
                noise = torch.nn.functional.dropout(noise, p=noise_dropout)
            return ops.cfg_dpmpp_2m_sde_step(x.contiguous(), m_c.contiguous(), None if m_u is None else m_u.contiguous(), noise, scale, a_t,
                                             float(np.sqrt(1.0 - a_t)), float(k_x[k]), float(k_d[k]), float(k_p[k]), float(k_n[k]), d=d,
                                             v_prediction=self.model.parameterization == "v")
        return ops.cfg_dpmpp_2m_step(x.contiguous(), m_c.contiguous(), None if m_u is None else m_u.contiguous(), scale, a_t,
                                     float(np.sqrt(1.0 - a_t)), float(k_x[k]), float(k_d[k]), float(k_p[k]), d=d,
                                     v_prediction=self.model.parameterization == "v")

    def _run(self, x, c, uc, scale, timesteps, alphas, k_x, k_d, k_p, mask=None, x0=None, callback=None, img_callback=None,
             ucg_schedule=None, log_every_t=100, intermediates=None, k_n=None, temperature=1., noise_dropout=0., plan=None):
        """the per-step path over a run of steps that starts without history (k_p[0] == 0); plan: the control modes of every step
        (`ddim_hacked.control_plan`), set before the step's model call"""
        total = len(timesteps)
        d = torch.empty_like(x, memory_format=torch.contiguous_format)
        for k in range(total):
            index = total - k - 1
            if mask is not None:
                ts = torch.full((x.shape[0],), int(timesteps[k]), device=x.device, dtype=torch.long)
                x = self.model.q_sample(x0, ts) * mask + (1. - mask) * x
            if ucg_schedule is not None:
                assert len(ucg_schedule) == total
                scale = ucg_schedule[k]
            with dh.cs.step_modes(self.model, plan, k):
                x = self._step(x, d, c, uc, scale, k, timesteps, alphas, k_x, k_d, k_p, k_n, temperature, noise_dropout)
            if callback:
                callback(k)
            if img_callback:
                img_callback(d.clone(), k)
            if intermediates is not None and (index % log_every_t == 0 or index == total - 1):
                intermediates["x_inter"].append(x)
                intermediates["pred_x0"].append(d.clone())
        return x

    # ------------------------------------------------------------------------------------------ whole-loop graph
    def _loop_graph_ok(self, img, c, uc, scale, total_steps):
        """the gating of `DDIMSampler._loop_graph_ok`, the bound of the library's timestep table included (the stochastic subclass's
        temperature / noise_dropout are ruled out by `sample`)"""
        return bool(dh.USE_GRAPH and dh.USE_LOOP_GRAPH and img.is_cuda and 2 <= total_steps <= dh.MAX_TABLE_STEPS
                    and (self._pair._fusable(c, uc, scale) or self._pair._unguided(c, uc, scale))
                    and self.model.parameterization in ("eps", "v"))

    def _loop_graphed(self, img, c, uc, scale, total_steps, log_every_t, intermediates, mask=None, x0=None):
        """`ddim_hacked.captured_loop` over this solver's steps: `_step` for the eager step 1, sdeo_dpmpp_2m_step for the captured ones
        (with a mask sdeo_dpmpp_2m_step_masked; the stochastic subclass's steps with k_n[i] != 0 sdeo_dpmpp_2m_sde_step, which reads
        its noise row by address).  The solver's only state next to x is D of the last step taken (self._loop_d)."""
        m, rt = self.model, self.model.rt
        ts, a_t, k_x, k_d, k_p, k_n = self.timesteps, self.alphas, self.k_x, self.k_d, self.k_p, self.k_n
        time_range = tuple(int(t) for t in ts)
        ident = DDIMSampler._ident
        unguided = self._pair._unguided(c, uc, scale)       # no guidance: the same steps with unguided=True on the b latents
        hint_shared = not unguided and ident(c["c_concat"]) == ident(uc["c_concat"])
        per_graph = dh.LOOP_GRAPH_STEPS if dh.LOOP_GRAPH_STEPS > 0 else total_steps
        shape_key = (tuple(img.shape), time_range, float(scale), int(log_every_t), m.scales_key(),
                     bool(m.only_mid_control), self._schedule_key, per_graph, hint_shared, m.parameterization,
                     None if mask is None else tuple(mask.shape), unguided, dh.ip_key(m), dh.freeu_key(m))
        live = [k_n is not None and float(k_n[i]) != 0. for i in range(total_steps)]
        plan = dh.control_plan(self._pair, c, uc, scale, total_steps)      # the control schedule, as in `DDIMSampler._loop_graphed`
        shape_key += (dh.loop_modes_key(m, plan),)

        def first_step(img, d):
            with dh.cs.step_modes(m, plan, 0):
                x1 = self._step(img, d, c, uc, scale, 0, ts, a_t, k_x, k_d, k_p, k_n)
            return x1, d.clone()

        def emit(i, staged, noise_row, blend):
            a = float(a_t[i])
            x, d = self._loop_x, self._loop_d
            head = (i, scale, a, float(np.sqrt(1.0 - a)), float(k_x[i]), float(k_d[i]), float(k_p[i]))
            kw = dict(hint_shared=hint_shared, v_prediction=m.parameterization == "v", unguided=unguided)
            with dh.cs.step_modes(m, plan, i):
                if noise_row is not None:
                    rt.dpmpp_2m_sde_step(x, d, noise_row, *head, float(k_n[i]), m.net0_scales(), m.only_mid_control, staged=staged, **kw,
                                         **(blend or {}))
                elif blend is None:
                    rt.dpmpp_2m_step(x, d, *head, m.net0_scales(), m.only_mid_control, staged=staged, **kw)
                else:
                    rt.dpmpp_2m_step_masked(x, d, *blend.values(), *head, m.net0_scales(), m.only_mid_control, **kw)

        return dh.captured_loop(self, img, mask, x0, time_range, live, shape_key, log_every_t, intermediates, "_loop_d", first_step, emit)

    # ------------------------------------------------------------------------------------------ img2img
    @torch.no_grad()
    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None):
        """`DDIMSampler.stochastic_encode` on this sampler's grid: index t counts grid points from the low-noise end (index 0 is the
        last timestep the loop visits), as ddim_alphas[t] does."""
        if use_original_steps:
            raise NotImplementedError("stochastic_encode works on the solver's own grid (use_original_steps is DDIM's)")
        asc = np.ascontiguousarray(self.alphas[::-1])
        sqrt_ac = torch.as_tensor(np.sqrt(asc), dtype=torch.float32, device=x0.device)
        sqrt_1m = torch.as_tensor(np.sqrt(1.0 - asc), dtype=torch.float32, device=x0.device)
        if noise is None:
            noise = torch.randn_like(x0)
        ext = lambda a: a[t.to(x0.device)].reshape(-1, *([1] * (x0.dim() - 1)))
        return ext(sqrt_ac) * x0 + ext(sqrt_1m) * noise

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None, use_original_steps=False,
               callback=None):
        """`DDIMSampler.decode`: the last t_start steps of the grid.  The run has no history, so it restarts at first order."""
        if use_original_steps:
            raise NotImplementedError("decode works on the solver's own grid (use_original_steps is DDIM's)")
        total = self.timesteps.shape[0]
        assert 0 <= t_start <= total
        if t_start == 0:
            return x_latent
        first = total - t_start
        alphas, alphas_next = self.alphas[first:], self.alphas_next[first:]
        k_x, k_d, k_p, k_n = self._coefficients(alphas, alphas_next)
        self._pair._cache_key = None
        x = x_latent.to(device=self.model.device, dtype=torch.float32)
        # a control schedule counts its window on the whole grid: decode walks its last t_start steps
        plan = dh.control_plan(self._pair, cond, unconditional_conditioning, unconditional_guidance_scale, total)
        return self._run(x, cond, unconditional_conditioning, unconditional_guidance_scale, self.timesteps[first:], alphas, k_x, k_d, k_p,
                         callback=callback, k_n=k_n, plan=None if plan is None else plan[first:])


class DPMSolverSDESampler(DPMSolverSampler):
    """DPM-Solver++(2M) SDE with the surface of `DPMSolverSampler` (sample / stochastic_encode / decode): eta in [0, 1] scales the noise
    each step injects (the module's docstring has the update).  eta = 0 takes the parent's code path: the same calls, the same bits.
    The grid defaults to log-SNR; the uniform-t grid is accepted but not usable at low step counts (see the module's docstring).
    temperature != 1 or noise_dropout != 0 run one step at a time, with `DDIMSampler`'s meaning."""

    def __init__(self, model, discretize="logsnr", lower_order_final=True, **kwargs):
        super().__init__(model, discretize=discretize, lower_order_final=lower_order_final, **kwargs)
        self.eta = 0.0

    @staticmethod
    def _check_eta(eta):
        eta = float(eta)
        if not 0.0 <= eta <= 1.0:
            raise ValueError(f"eta = {eta}: DPM-Solver++(2M) SDE takes eta in [0, 1] (0: the ODE solver, 1: the full SDE noise)")
        return eta

    def make_schedule(self, ddim_num_steps, ddim_eta=None, verbose=True):
        """the parent's grid; the coefficients are `sde_coefficients` at ddim_eta (the parent's own at 0).  ddim_eta stays in force, for
        `decode` and for a call without it, until another one is given."""
        eta = self.eta if ddim_eta is None else self._check_eta(ddim_eta)
        if eta != self.eta:
            self._schedule_key = None          # the parent's keys do not know eta: new coefficients, and new graphs that bake them in
            self._loop_key = None
            self.eta = eta
        super().make_schedule(ddim_num_steps, verbose=verbose)

    def _coefficients(self, alphas, alphas_next):
        if self.eta == 0.0:
            return super()._coefficients(alphas, alphas_next)
        return sde_coefficients(alphas, alphas_next, self.eta, self.lower_order_final)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, eta=0., verbose=True, **kwargs):
        """`DPMSolverSampler.sample` with eta in [0, 1]"""
        self.make_schedule(S, ddim_eta=self._check_eta(eta), verbose=verbose)
        return super().sample(S, batch_size, shape, conditioning, eta=0., verbose=verbose, **kwargs)
