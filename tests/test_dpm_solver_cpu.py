"""DPM-Solver++(2M) without a GPU: the fp64 oracle's own identities (first order == eta-0 DDIM, convergence on a Gaussian model whose
probability-flow ODE has a closed form), the product's step grid and host coefficients against the oracle, and the two new C-ABI
entry points as the header declares them."""
import ctypes

import numpy as np
import pytest
import torch

from tests import dpm_oracle as D

AC = D.sd_alphas_cumprod()


def test_first_order_step_is_the_eta0_ddim_step():
    rng = np.random.RandomState(0)
    x, e = rng.randn(257), rng.randn(257)
    for a_t, a_next in ((AC[999], AC[888]), (AC[597], AC[413]), (AC[11], AC[2]), (AC[2], AC[0]), (0.31, 0.62)):
        d = D.data_prediction(x, e, None, 1.0, a_t)
        got, ref = D.first_order(x, d, a_t, a_next), D.ddim_eta0(x, e, a_t, a_next)
        assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
        (k_x, k_d, k_p), = D.coefficients([a_t], [a_next])
        assert k_p == 0.0 and np.abs(k_x * x + k_d * d - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def test_folded_coefficients_restate_the_second_order_step():
    rng = np.random.RandomState(1)
    x, d, d_prev = rng.randn(64), rng.randn(64), rng.randn(64)
    ts, a_t, a_next = D.grid(AC, 10, "logsnr")
    co = D.coefficients(a_t, a_next, lower_order_final=False)
    for k in range(1, 10):
        ref = D.second_order(x, d, d_prev, a_t[k], a_next[k], a_t[k - 1])
        k_x, k_d, k_p = co[k]
        assert k_p < 0.0 < k_d
        assert np.abs(k_x * x + k_d * d + k_p * d_prev - ref).max() <= 1e-12


@pytest.mark.parametrize("S", [5, 10, 20, 30, 50, 100])
def test_logsnr_grid(S):
    from stablediffusioneo_amd.cldm.dpm_solver import make_logsnr_timesteps
    ts = make_logsnr_timesteps(AC, S)
    assert len(ts) == S and int(ts[0]) == len(AC) - 1
    assert all(int(a) > int(b) for a, b in zip(ts[:-1], ts[1:])) and int(ts[-1]) >= 1
    assert [int(t) for t in ts] == D.logsnr_timesteps(AC, S)
    if S == 10:
        assert [int(t) for t in ts[:4]] == [999, 888, 757, 597] and [int(t) for t in ts[-3:]] == [36, 11, 2]


class _Schedule:
    """what make_schedule reads of a model"""
    num_timesteps = 1000
    parameterization = "eps"
    device = torch.device("cpu")
    alphas_cumprod = torch.tensor(AC, dtype=torch.float32)


@pytest.mark.parametrize("discretize", ["logsnr", "uniform"])
@pytest.mark.parametrize("lower_order_final", [True, False])
def test_make_schedule_against_the_oracle(discretize, lower_order_final):
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler
    s = DPMSolverSampler(_Schedule(), discretize=discretize, lower_order_final=lower_order_final)
    ac = _Schedule.alphas_cumprod.double().numpy()
    for S in (5, 10, 20):
        s.make_schedule(S, verbose=False)
        ts, a_t, a_next = D.grid(ac, S, discretize)
        assert [int(t) for t in s.timesteps] == ts
        np.testing.assert_allclose(s.alphas, a_t, rtol=1e-15)
        np.testing.assert_allclose(s.alphas_next, a_next, rtol=1e-15)
        ref = np.asarray(D.coefficients(a_t, a_next, lower_order_final))
        for got, col in ((s.k_x, 0), (s.k_d, 1), (s.k_p, 2)):
            assert got.dtype == np.float64
            np.testing.assert_allclose(got, ref[:, col], rtol=1e-12, atol=0)
        assert s.k_p[0] == 0.0 and (s.k_p[-1] == 0.0) == lower_order_final
    kept = s.timesteps
    s.make_schedule(20, verbose=False)
    assert s.timesteps is kept                        # same arguments, same model schedule: the arrays are kept


def test_deterministic_only():
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler
    s = DPMSolverSampler(_Schedule())
    for kw in ({"eta": 0.5}, {"score_corrector": object()}, {"quantize_x0": True}, {"dynamic_threshold": 0.9}):
        with pytest.raises(NotImplementedError, match="deterministic"):
            s.sample(5, 1, (4, 8, 8), None, verbose=False, **kw)
    with pytest.raises(NotImplementedError):
        DPMSolverSampler(_Schedule(), discretize="quad")


def _gaussian_errors(s2):
    x_T = np.random.RandomState(7).randn(512)
    model = lambda a_of: (lambda x, t: (D.gaussian_eps(x, a_of[t], s2), None, 1.0))
    a_of = {t: float(AC[t]) for t in range(len(AC))}
    errs = {}
    for S in (10, 20):
        ts, a_t, a_next = D.grid(AC, S, "logsnr")
        x = D.sample(model(a_of), x_T, ts, a_t, a_next)[-1]
        errs["2m", S] = D.rel_max_err(x, D.gaussian_exact(x_T, a_next[-1], a_t[0], s2))
    ts, a_t, a_next = D.grid(AC, 20, "uniform")
    x = D.ddim_sample(model(a_of), x_T, ts, a_t, a_next)
    errs["ddim", 20] = D.rel_max_err(x, D.gaussian_exact(x_T, a_next[-1], a_t[0], s2))
    return errs


@pytest.mark.parametrize("s2", [0.25, 1.0])
def test_convergence_on_the_gaussian_model(s2):
    """each sampler against the exact ODE solution between its own end points"""
    e = _gaussian_errors(s2)
    print(f"[dpm] s2={s2}: DDIM uniform S=20 {e['ddim', 20]:.4g}; 2M logsnr S=10 {e['2m', 10]:.4g}, S=20 {e['2m', 20]:.4g}")
    assert e["2m", 10] <= 0.5 * e["ddim", 20]
    assert e["2m", 20] < e["2m", 10]


def test_new_entry_points_are_declared_typed_and_exported():
    from stablediffusioneo_amd import _lib, build
    protos = _lib.prototypes(_lib.HEADER)
    V, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert protos["sdeo_cfg_dpmpp_2m_step"] == (I, [V] * 5 + [F] * 6 + [I, ctypes.c_int64, V])
    assert protos["sdeo_dpmpp_2m_step"] == (I, [V, V, V, I] + [F] * 6 + [V, I, I, V])
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.sdeo_version() == 101
    for name in ("sdeo_cfg_dpmpp_2m_step", "sdeo_dpmpp_2m_step"):
        fn = getattr(lib, name)
        assert fn.restype is protos[name][0] and list(fn.argtypes) == protos[name][1]
    # host-side validation, before any launch: a_t <= 0, non-finite coefficients, k_p != 0 without d
    p = ctypes.c_void_p(16)
    call = lambda d, a_t, k_x, k_d, k_p: lib.sdeo_cfg_dpmpp_2m_step(p, d, p, p, None, 7.5, a_t, 0.5, k_x, k_d, k_p, 0, 64, None)
    assert call(p, 0.0, 1.0, 1.0, 0.0) != 0 and b"a_t" in lib.sdeo_last_error()
    assert call(p, 0.5, float("nan"), 1.0, 0.0) != 0 and b"non-finite" in lib.sdeo_last_error()
    assert call(p, 0.5, 1.0, float("inf"), 0.0) != 0 and b"non-finite" in lib.sdeo_last_error()
    assert call(None, 0.5, 1.0, 1.0, -0.25) != 0 and b"d is null" in lib.sdeo_last_error()
    assert lib.sdeo_dpmpp_2m_step(None, p, p, 0, 7.5, 0.5, 0.5, 1.0, 1.0, 0.0, None, 0, 0, None) != 0
