"""The LCM sampler on the host: its grid, the boundary condition, its coefficient arrays against the step-by-step restatement
(tests/lcm_oracle.py) and on the Gaussian problem, where the consistency function is known in closed form; and the new step flag in the
header and the runtime.  No GPU."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

from tests import dpm_oracle as D
from tests import lcm_oracle as LO

AC = D.sd_alphas_cumprod()
ROOT = Path(__file__).resolve().parent.parent


class _Model:
    """what the samplers read of a model on the host"""
    num_timesteps = 1000
    parameterization = "eps"
    device = "cpu"

    def __init__(self):
        import torch
        self.alphas_cumprod = torch.from_numpy(AC)


def _sampler(S, **kw):
    from stablediffusioneo_amd.cldm.lcm import LCMSampler
    s = LCMSampler(_Model(), **kw)
    s.make_schedule(S, verbose=False)
    return s


# ------------------------------------------------------------------------------------------ grid
def test_grid():
    from stablediffusioneo_amd.cldm.lcm import lcm_timesteps
    assert lcm_timesteps(1000, 4).tolist() == [999, 759, 519, 279]
    assert lcm_timesteps(1000, 1).tolist() == [999]
    assert lcm_timesteps(1000, 6).tolist() == [999, 839, 679, 519, 359, 199]
    full = lcm_timesteps(1000, 50).tolist()
    assert len(full) == 50 and full[0] == 999 and full[-1] == 19 and all(a - b == 20 for a, b in zip(full, full[1:]))
    for bad in (51, 0, -1):
        with pytest.raises(ValueError):
            lcm_timesteps(1000, bad)
    for S in (1, 2, 3, 4, 5, 6, 7, 8, 25, 50):
        assert lcm_timesteps(1000, S).tolist() == LO.timesteps(1000, S) == _sampler(S).timesteps.tolist()
    with pytest.raises(ValueError):
        _sampler(51)
    with pytest.raises(ValueError):
        _sampler(0)


def test_constructor_defaults_and_surface():
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler
    from stablediffusioneo_amd.cldm.lcm import LCMSampler
    s = LCMSampler(_Model())
    assert isinstance(s, DPMSolverSampler)
    assert (s.original_steps, s.timestep_scaling, s.sigma_data) == (50, 10.0, 0.5)
    for name in ("sample", "stochastic_encode", "decode", "make_schedule"):
        assert callable(getattr(s, name))
    for bad in (0.5, 1.0):
        with pytest.raises(NotImplementedError, match="eta"):
            s.make_schedule(4, ddim_eta=bad, verbose=False)
        with pytest.raises(NotImplementedError, match="eta"):
            s.sample(4, 1, (4, 8, 8), None, eta=bad, verbose=False)


# ------------------------------------------------------------------------------------------ boundary condition and coefficients
def test_boundary():
    from stablediffusioneo_amd.cldm.lcm import boundary_scalings
    c_skip, c_out = boundary_scalings(0)
    assert c_skip == 1.0 and c_out == 0.0
    assert LO.scalings(0) == (1.0, 0.0)
    for S in (1, 2, 4, 8):
        s = _sampler(S)
        assert s.k_n[-1] == 0.0 and (s.k_n[:-1] > 0).all() and (s.k_p == 0.0).all()
        assert s.alphas_next[-1] == 1.0 and np.array_equal(s.alphas_next[:-1], AC[s.timesteps[1:]])
        assert np.array_equal(s.alphas, AC[s.timesteps])


@pytest.mark.parametrize("S", [1, 2, 4, 6, 8, 50])
def test_coefficients_are_the_restated_step(S):
    """k_x x + k_d D + k_n n against denoise-then-renoise, on numbers"""
    s = _sampler(S)
    ts, a_t, a_next = LO.grid(AC, S)
    x, d, n = 0.7, -1.3, 0.4
    for k in range(S):
        want = LO.step(x, d, n, ts[k], a_next[k])
        got = s.k_x[k] * x + s.k_d[k] * d + s.k_p[k] * 9.0 + s.k_n[k] * n
        assert abs(got - want) <= 1e-15 * max(1.0, abs(want)) * 4


def test_decode_tail_coefficients():
    """`decode` restarts on the last t_start steps: their coefficients are the tail of the full run's (the scalings follow the timestep)"""
    s = _sampler(6)
    for t_start in (1, 3, 6):
        first = 6 - t_start
        tail = s._coefficients(s.alphas[first:], s.alphas_next[first:])
        for got, want in zip(tail, (s.k_x, s.k_d, s.k_p, s.k_n)):
            assert np.array_equal(got, want[first:])


@pytest.mark.parametrize("s2", [0.25, 1.0, 4.0])
@pytest.mark.parametrize("S", [1, 2, 4, 6, 8, 50])
def test_exact_consistency_on_the_gaussian_problem(S, s2):
    """data ~ N(0, s2 I): f(x, t) = x s / sqrt(a_t s2 + 1 - a_t).  With the model whose D satisfies c_skip x + c_out D = f, the marginal
    variance after every step is a_next s2 + 1 - a_next: algebra, so the bound is rounding (4e-16 observed in numpy on the SD schedule,
    1e-12 asserted)."""
    s = _sampler(S)
    ts, a_t, a_next = LO.grid(AC, S)
    pairs = LO.gaussian_variances(ts, a_t, a_next, s.k_x, s.k_d, s.k_n, s2)
    err = max(abs(v / e - 1.0) for v, e in pairs)
    print(f"[lcm] Gaussian s2={s2} S={S}: max relative variance error {err:.2e}")
    assert len(pairs) == S and err <= 1e-12
    assert pairs[-1][1] == s2                       # the last step returns the denoised latent: the data's own variance


# ------------------------------------------------------------------------------------------ ABI
def _header_define(name):
    text = (ROOT / "include" / "sdeo.h").read_text()
    m = re.search(rf"^#define {name} (\d+)$", text, re.M)
    assert m, name
    return int(m.group(1))


def test_flag_in_header_and_runtime():
    from stablediffusioneo_amd import runtime
    assert _header_define("SDEO_STEP_UNGUIDED") == 128
    assert _header_define("SDEO_ABI_VERSION") == 101
    assert runtime.STEP_UNGUIDED == _header_define("SDEO_STEP_UNGUIDED")
    flags = [_header_define(n) for n in ("SDEO_STEP_LATENT_STAGED", "SDEO_STEP_HINT_SHARED", "SDEO_STEP_V_PREDICTION", "SDEO_STEP_UNGUIDED")]
    assert flags == [runtime.STEP_LATENT_STAGED, runtime.STEP_HINT_SHARED, runtime.STEP_V_PREDICTION, runtime.STEP_UNGUIDED]
    assert len({f for f in flags}) == 4 and all(f & (f - 1) == 0 and f < 256 for f in flags)       # single bits below SDEO_TIMESTEP_ROW's row
    assert runtime.SdeoRuntime._step_flags(True, False, True, 0, True) == 16 | 64 | 128
    assert runtime.SdeoRuntime._step_flags(False, True, False) == 32


def test_unguided_refusals_that_need_no_device():
    """the flag does not get past a null handle, and the coefficient checks still come first, in the entry point's name"""
    import ctypes
    from stablediffusioneo_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.sdeo_version() == 101
    p = ctypes.c_void_p(256)
    rc = lib.sdeo_ddim_step_eta(None, p, p, None, 0.3, None, None, None, 0, 0, 0.0, 0.0, 1, float("nan"), 0.31, 0.62, 0.83, None, 0, 128, None)
    assert rc != 0 and lib.sdeo_last_error().startswith(b"sdeo_ddim_step_eta") and b"noise is null" in lib.sdeo_last_error()
    # cfg_scale is neither read nor checked: a NaN passes the coefficient checks of an unguided step (and stops at the null handle)
    rc = lib.sdeo_dpmpp_2m_sde_step(None, p, p, p, None, None, None, 0, 0, 0.0, 0.0, 1, float("nan"), 0.31, 0.83, 0.9, 0.1, 0.0, 0.2, None, 0, 128,
                                    None)
    assert rc != 0 and b"null handle" in lib.sdeo_last_error()
    rc = lib.sdeo_dpmpp_2m_sde_step(None, p, p, p, None, None, None, 0, 0, 0.0, 0.0, 1, float("nan"), 0.31, 0.83, 0.9, 0.1, 0.0, 0.2, None, 0, 0,
                                    None)
    assert rc != 0 and b"non-finite" in lib.sdeo_last_error()


def test_sampler_name():
    import inspect
    from stablediffusioneo_amd import canny2image as c2i
    src = inspect.getsource(c2i.hackathon._init_model)
    assert '"lcm"' in src and "LCMSampler" in src
    doc = c2i.hackathon.initialize.__doc__
    assert "2-8 steps" in doc and "cond_proj" in doc and "guidance embedding" in doc
