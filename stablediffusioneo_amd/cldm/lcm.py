"""Latent Consistency Model sampling (Luo et al. 2023, "Latent Consistency Models"; the LCM-LoRA report of the same authors) with the
surface of `DPMSolverSampler`: the multistep consistency sampler for 2-8 steps, for SD-1.5 / SD-2.x weights with an LCM-LoRA merged in
(`lora.apply_lora`).  LCM-LoRA has no guidance embedding, so the guidance scale keeps its classifier-free meaning: 1.0 (no
unconditional branch) is the canonical setting, 1-2 the useful range.  Full LCM checkpoints with `time_embedding.cond_proj` (the
guidance-embedded distillation) are not supported; the loader's unknown-key report refuses them.

A step at timestep t with data prediction D (the pred_x0 of the DDIM kernels, CFG-combined when guided) evaluates the consistency
function through the boundary-condition scalings and re-noises to the next grid point:

    c_skip = sd^2 / ((s t)^2 + sd^2),   c_out = s t / sqrt((s t)^2 + sd^2)          s = timestep_scaling, sd = sigma_data
    denoised = c_skip x + c_out D
    x_next   = sqrt(a_next) denoised + sqrt(1 - a_next) noise,    noise ~ N(0, I) drawn per step;   a_next = 1 after the last step

which is the linear update x_next = k_x x + k_d D + k_p D_prev + k_n noise of `sdeo_dpmpp_2m_sde_step` with k_p = 0:

    k_x = sqrt(a_next) c_skip,   k_d = sqrt(a_next) c_out,   k_n = sqrt(1 - a_next)       (k_n = 0 on the last step: it draws nothing)

So the sampler is coefficients only.  The loop, the graph of steps 2..S, the noise rows and their draw order (`ddim_hacked.draw_rows`)
and the mask / x0 branch are the parent's; with guidance the captured steps are the CFG-pair steps, without it the un-paired ones
(SDEO_STEP_UNGUIDED).  There is no eta: eta != 0 is refused; temperature != 1 and noise_dropout keep the per-step loop, as in
`DPMSolverSDESampler`.

The grid is the LCM authors' rule: the `original_steps` training timesteps origin = k, 2k, ... (minus one), k = T // original_steps,
walked from the top in strides of original_steps // S; S = 4 on T = 1000 gives [999, 759, 519, 279]."""
from __future__ import annotations

import numpy as np
import torch

from .dpm_solver import DPMSolverSampler


def lcm_timesteps(num_timesteps, S, original_steps=50):
    """the S timesteps (decreasing) of an S-step LCM run on a model of num_timesteps training steps"""
    S, original_steps = int(S), int(original_steps)
    k = int(num_timesteps) // original_steps
    if k < 1:
        raise ValueError(f"original_steps = {original_steps} on a schedule of {num_timesteps} timesteps")
    if not 1 <= S <= original_steps:
        raise ValueError(f"{S} steps: the LCM grid takes 1 to original_steps = {original_steps}")
    origin = np.arange(1, original_steps + 1, dtype=np.int64) * k - 1
    return np.ascontiguousarray(origin[::-(original_steps // S)][:S])


def boundary_scalings(t, timestep_scaling=10.0, sigma_data=0.5):
    """(c_skip, c_out) of the consistency parameterisation at timestep t, fp64; c_skip(0) = 1 and c_out(0) = 0"""
    st = np.asarray(t, dtype=np.float64) * float(timestep_scaling)
    sd2 = float(sigma_data) ** 2
    return sd2 / (st * st + sd2), st / np.sqrt(st * st + sd2)


def lcm_coefficients(timesteps, alphas_next, timestep_scaling=10.0, sigma_data=0.5):
    """(k_x, k_d, k_p, k_n) fp64 arrays of a run of LCM steps at `timesteps` that land on alphas_next"""
    a_n = np.asarray(alphas_next, dtype=np.float64)
    c_skip, c_out = boundary_scalings(timesteps, timestep_scaling, sigma_data)
    return np.sqrt(a_n) * c_skip, np.sqrt(a_n) * c_out, np.zeros_like(a_n), np.sqrt(1.0 - a_n)


class LCMSampler(DPMSolverSampler):
    """The multistep LCM sampler: `sample` / `stochastic_encode` / `decode` of `DPMSolverSampler` on the LCM grid with the LCM
    coefficients.  Meant for 2-8 steps at a guidance scale of 1-2 on weights with an LCM-LoRA merged in."""

    def __init__(self, model, original_steps=50, timestep_scaling=10.0, sigma_data=0.5, **kwargs):
        super().__init__(model, **kwargs)
        self.original_steps = int(original_steps)
        self.timestep_scaling = float(timestep_scaling)
        self.sigma_data = float(sigma_data)

    @staticmethod
    def _no_eta(eta):
        if eta is not None and eta != 0.:
            raise NotImplementedError(f"the LCM sampler has no eta (every step but the last re-noises in full): eta = {eta} is not available")

    def make_schedule(self, ddim_num_steps, ddim_eta=0., verbose=True):
        """the parent's arrays on the LCM grid: timesteps, alphas (a_t), alphas_next (1.0 after the last step) and the coefficients;
        cached by the arguments and the identity of the model's schedule, as there"""
        self._no_eta(ddim_eta)
        ac = self.model.alphas_cumprod
        fp = (id(ac), int(getattr(ac, "_version", 0)), int(ac.data_ptr()) if isinstance(ac, torch.Tensor) else 0, tuple(ac.shape))
        key = (int(ddim_num_steps), "lcm", self.original_steps, self.timestep_scaling, self.sigma_data, id(self.model),
               self.ddpm_num_timesteps, fp)
        if self._schedule_key == key:
            return
        self._schedule_key = None
        acn = ac.detach().double().cpu().numpy() if isinstance(ac, torch.Tensor) else np.asarray(ac, dtype=np.float64)
        assert acn.shape[0] == self.ddpm_num_timesteps, "alphas have to be defined for each timestep"
        ts = lcm_timesteps(self.ddpm_num_timesteps, ddim_num_steps, self.original_steps)
        if verbose:
            print(f"Selected timesteps for the LCM sampler: {ts}")
        self.timesteps = ts
        self.alphas = acn[ts]
        self.alphas_next = np.append(acn[ts[1:]], 1.0)
        self.k_x, self.k_d, self.k_p, self.k_n = self._coefficients(self.alphas, self.alphas_next)
        self._schedule_key = key

    def _coefficients(self, alphas, alphas_next):
        """of the run made of the last len(alphas) steps of the grid (the whole grid, or `decode`'s tail of it): the scalings depend
        on the timestep itself, which the parent's signature does not carry"""
        ts = self.timesteps[len(self.timesteps) - len(alphas):]
        return lcm_coefficients(ts, alphas_next, self.timestep_scaling, self.sigma_data)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, eta=0., **kwargs):
        """`DPMSolverSampler.sample`; eta != 0 raises"""
        self._no_eta(eta)
        return super().sample(S, batch_size, shape, conditioning, eta=0., **kwargs)
