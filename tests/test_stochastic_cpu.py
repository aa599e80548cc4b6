"""The stochastic samplers without a GPU: the fp64 oracle's identities (tests/sde_oracle.py), closed-form variance propagation on the
Gaussian problem, the host-side coefficients of `DPMSolverSDESampler` against the oracle, the three new C symbols and the sampler name.

The variance figures (computed from the formulas of the issue, printed by the test): on the log-SNR grid the second-order run ends between
+1.9e-2 and +8.3e-2 of the exact variance, the all-first-order run between -0.20 and -0.43, smallest ratio 5.2 (s2 = 4, S = 10, eta = 1);
on the uniform-t grid at S = 10, s2 = 0.25, eta = 1 the second-order figure is +1.09 -- the reason for the sampler's default grid."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import dpm_oracle as D
from tests import sde_oracle as SO

AC = D.sd_alphas_cumprod()


# ------------------------------------------------------------------------------------------ oracle identities
def test_first_order_eta1_is_the_eta1_ddim_step():
    _, a_t, a_next = D.grid(AC, 20, "uniform")
    worst = 0.0
    for k, (k_x, k_d, k_p, k_n) in enumerate(SO.coefficients(a_t, a_next, 1.0, second_order=False)):
        assert k_p == 0.0
        d_x, d_d, d_n = SO.ddim_coefficients(a_t[k], a_next[k], 1.0)
        worst = max(worst, abs(k_x - d_x) / abs(d_x), abs(k_d - d_d) / abs(d_d), abs(k_n - d_n) / d_n)
    print(f"[sde] first-order eta = 1 against DDIM eta = 1, S = 20 uniform: max relative coefficient difference {worst:.2e}")
    assert worst < 1e-12


@pytest.mark.parametrize("discretize", ["logsnr", "uniform"])
@pytest.mark.parametrize("lower_order_final", [True, False])
def test_eta0_is_the_ode_solver(discretize, lower_order_final):
    _, a_t, a_next = D.grid(AC, 10, discretize)
    ode = D.coefficients(a_t, a_next, lower_order_final)
    sde = SO.coefficients(a_t, a_next, 0.0, lower_order_final)
    assert [c[:3] for c in sde] == ode and all(c[3] == 0.0 for c in sde)


def test_step_matches_its_coefficients():
    g = np.random.default_rng(3)
    x, d, d_prev, n = (g.standard_normal(16) for _ in range(4))
    a = [0.12, 0.31, 0.62]
    (_, _, _, _), (k_x, k_d, k_p, k_n) = SO.coefficients(a[:2], a[1:], 0.7, lower_order_final=False)
    np.testing.assert_allclose(SO.step(x, d, d_prev, n, a[1], a[2], a[0], 0.7), k_x * x + k_d * d + k_p * d_prev + k_n * n, rtol=1e-13)
    assert k_p != 0.0 and k_n > 0.0


# ------------------------------------------------------------------------------------------ variance propagation, closed form
@pytest.mark.parametrize("eta", [0.5, 1.0])
@pytest.mark.parametrize("S", [10, 20])
@pytest.mark.parametrize("s2", [0.25, 1.0, 4.0])
def test_second_order_keeps_the_variance(s2, S, eta):
    e2 = SO.gaussian_final_variance_error(S, "logsnr", eta, s2)
    e1 = SO.gaussian_final_variance_error(S, "logsnr", eta, s2, second_order=False)
    print(f"[sde] variance s2={s2} S={S} eta={eta} logsnr: second order {e2:+.3e}, first order {e1:+.3e}, ratio {abs(e1) / abs(e2):.2f}")
    assert abs(e2) <= 0.1
    assert abs(e2) * 4.0 <= abs(e1)


def test_uniform_grid_is_worse_at_low_step_counts():
    uni = SO.gaussian_final_variance_error(10, "uniform", 1.0, 0.25)
    log = SO.gaussian_final_variance_error(10, "logsnr", 1.0, 0.25)
    print(f"[sde] variance s2=0.25 S=10 eta=1: uniform {uni:+.3e}, logsnr {log:+.3e}")
    assert abs(uni) > abs(log)


# ------------------------------------------------------------------------------------------ product code
@pytest.mark.parametrize("eta", [0.3, 1.0])
@pytest.mark.parametrize("S,discretize,lower_order_final", [(10, "logsnr", True), (20, "uniform", True), (7, "logsnr", False)])
def test_sde_coefficients_match_the_oracle(S, discretize, lower_order_final, eta):
    from stablediffusioneo_amd.cldm.dpm_solver import sde_coefficients
    _, a_t, a_next = D.grid(AC, S, discretize)
    got = sde_coefficients(a_t, a_next, eta, lower_order_final)
    assert len(got) == 4 and all(g.dtype == np.float64 and g.shape == (S,) for g in got)
    want = np.asarray(SO.coefficients(a_t, a_next, eta, lower_order_final)).T
    for g, w in zip(got, want):
        np.testing.assert_allclose(g, w, rtol=1e-12, atol=0.0)
    assert (got[3] > 0).all() and (got[2][1:S - 1] != 0).all()


@pytest.mark.parametrize("lower_order_final", [True, False])
def test_sde_coefficients_at_eta0_are_the_ode_solvers_bits(lower_order_final):
    from stablediffusioneo_amd.cldm.dpm_solver import multistep_coefficients, sde_coefficients
    _, a_t, a_next = D.grid(AC, 10, "logsnr")
    k = sde_coefficients(a_t, a_next, 0.0, lower_order_final)
    for got, want in zip(k, multistep_coefficients(a_t, a_next, lower_order_final)):
        assert got.tobytes() == want.tobytes()
    assert (k[3] == 0.0).all()
    assert list(inspect.signature(sde_coefficients).parameters) == ["alphas", "alphas_next", "eta", "lower_order_final"]


def test_new_symbols_are_exported_and_typed():
    from stablediffusioneo_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.sdeo_version() == 101                       # no existing argument changed meaning
    V, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    names = _lib.declared_symbols()
    for n in ("sdeo_cfg_dpmpp_2m_sde_step", "sdeo_ddim_step_eta", "sdeo_dpmpp_2m_sde_step"):
        assert n in names and hasattr(lib, n), n
        assert getattr(lib, n).restype is I
    # x_next, d, x, m_c, m_u, noise | cfg_scale, a_t, sqrt_one_minus_at, k_x, k_d, k_p, k_n | flags, n, stream
    assert list(lib.sdeo_cfg_dpmpp_2m_sde_step.argtypes) == [V] * 6 + [F] * 7 + [I, ctypes.c_int64, V]
    # h, x, pred_x0, noise | sigma_t | orig, mask_noise, mask | mask_n, mask_c | sqrt_a, sqrt_one_minus_a | table_row | cfg_scale, a_t,
    # a_prev, sqrt_one_minus_at | host_control_scales | only_mid_control, flags | stream
    assert list(lib.sdeo_ddim_step_eta.argtypes) == [V] * 4 + [F] + [V] * 3 + [I] * 2 + [F] * 2 + [I] + [F] * 4 + [V] + [I] * 2 + [V]
    # h, x, d, noise, orig, mask_noise, mask | mask_n, mask_c | sqrt_a, sqrt_one_minus_a | table_row | cfg_scale, a_t, sqrt_one_minus_at,
    # k_x, k_d, k_p, k_n | host_control_scales | only_mid_control, flags | stream
    assert list(lib.sdeo_dpmpp_2m_sde_step.argtypes) == [V] * 7 + [I] * 2 + [F] * 2 + [I] + [F] * 7 + [V] + [I] * 2 + [V]
    # the entry points they extend keep their prototypes
    assert list(lib.sdeo_cfg_dpmpp_2m_step.argtypes) == [V] * 5 + [F] * 6 + [I, ctypes.c_int64, V]
    assert list(lib.sdeo_ddim_step.argtypes) == [V] * 3 + [I] + [F] * 4 + [V] + [I] * 2 + [V]


def test_refusals_that_need_no_device():
    """the unfused step checks its coefficients on the host before it launches anything"""
    from stablediffusioneo_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    rc = lib.sdeo_cfg_dpmpp_2m_sde_step(p, None, p, p, p, None, 7.5, 0.31, 0.83, 0.9, 0.1, 0.0, 0.2, 0, 64, None)
    assert rc != 0 and b"noise is null" in lib.sdeo_last_error()
    rc = lib.sdeo_cfg_dpmpp_2m_sde_step(p, None, p, p, p, p, 7.5, 0.31, 0.83, 0.9, 0.1, 0.0, float("inf"), 0, 64, None)
    assert rc != 0 and b"non-finite" in lib.sdeo_last_error()
    rc = lib.sdeo_ddim_step_eta(None, p, p, None, 0.3, None, None, None, 0, 0, 0.0, 0.0, 1, 7.5, 0.31, 0.62, 0.83, None, 0, 0, None)
    assert rc != 0 and b"noise is null" in lib.sdeo_last_error()
    rc = lib.sdeo_ddim_step_eta(None, p, p, p, 0.7, None, None, None, 0, 0, 0.0, 0.0, 1, 7.5, 0.31, 0.62, 0.83, None, 0, 0, None)
    assert rc != 0 and b"1 - a_prev - sigma_t^2 < 0" in lib.sdeo_last_error()


class _Model:
    """what the samplers read of a model on the host"""
    num_timesteps = 1000
    parameterization = "eps"
    device = "cpu"

    def __init__(self):
        import torch
        self.alphas_cumprod = torch.from_numpy(AC).float()


def test_sampler_eta_range_and_parent_refusal():
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler, DPMSolverSDESampler, multistep_coefficients, sde_coefficients
    s = DPMSolverSDESampler(_Model())
    assert s.discretize == "logsnr"
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="eta"):
            s.make_schedule(10, ddim_eta=bad, verbose=False)
        with pytest.raises(ValueError, match="eta"):
            s.sample(10, 1, (4, 8, 8), None, eta=bad, verbose=False)
    s.make_schedule(10, ddim_eta=1.0, verbose=False)
    for got, want in zip((s.k_x, s.k_d, s.k_p, s.k_n), sde_coefficients(s.alphas, s.alphas_next, 1.0)):
        assert np.array_equal(got, want)
    s.make_schedule(10, ddim_eta=0.0, verbose=False)           # eta = 0: the parent's coefficients, and no noise coefficients at all
    for got, want in zip((s.k_x, s.k_d, s.k_p), multistep_coefficients(s.alphas, s.alphas_next)):
        assert got.tobytes() == want.tobytes()
    assert s.k_n is None
    with pytest.raises(NotImplementedError):
        DPMSolverSampler(_Model()).make_schedule(10, ddim_eta=0.5, verbose=False)


def test_sampler_name():
    from stablediffusioneo_amd import canny2image as c2i
    src = inspect.getsource(c2i.hackathon._init_model)
    assert '"dpmpp_2m_sde"' in src and "DPMSolverSDESampler" in src
    with pytest.raises(ValueError, match="sampler"):
        c2i.hackathon()._init_model("synthetic:0", "tiny", None, sampler="euler_a")
