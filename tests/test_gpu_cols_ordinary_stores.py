"""GPU tier of the ORDINARY-store half of the device-column kernels (varpro_amd/csrc/vp_cols.hpp, vp_irf.hpp): every fill
and scan kernel exists with non-temporal stores (the library's default, what every other test runs) and with ordinary
stores (``set_column_fit(..., 0)``), and both halves are one body -- so the columns, and a fit made from them, must not
depend on the store kind, BIT FOR BIT.  One mixed descriptor reaches the pointwise kernel (Gauss, exponential decay,
constant) and the scan kernel (kinds 9, 10 and 11) in one launch sequence."""
import functools

import numpy as np
import pytest

import irf_cases as ic
import irf_periodic_cases as pc
import varpro_amd as vp
from varpro_amd import basis
from test_gpu_bounds import inside
from test_gpu_external import gauss
from test_gpu_peak_kinds import report_equal

pytestmark = pytest.mark.gpu
B = 12


def mixed_model(x, dtype=np.float64):
    """c1 Gauss(mu, s) + c2 exp(-t/tau) + c3 (irf * exp tau1) + c4 irf + c5 (irf * exp tau2, periodic) + c6
    (n = 6, q = 5, p = 5; pairs: mu, s | tau | tau1 | tau2)"""
    return (vp.SeparableModelBuilder(["mu", "s", "tau", "tau1", "tau2"], dtype=dtype)
            .function(["mu", "s"], basis.GAUSS).partial_deriv("mu").partial_deriv("s")
            .function(["tau"], basis.EXP_DECAY).partial_deriv("tau")
            .function(["tau1"], basis.EXP_DECAY_IRF).partial_deriv("tau1")
            .invariant_function(basis.IRF)
            .function(["tau2"], basis.EXP_DECAY_IRF_PERIODIC).partial_deriv("tau2")
            .invariant_function(basis.CONST)
            .independent_variable(x).initial_parameters([8.0, 0.6, 2.0, 0.8, 4.5]).build())


def mixed_case(m, dtype, seed=0):
    """(x, irf, alpha) on a uniform grid of step 12/128 (exactly representable in fp32): B parameter sets, every
    lifetime well inside the dtype's range"""
    rng = np.random.default_rng(4200 + m + seed)
    dt = 12.0 / 128.0
    x = (dt * np.arange(m)).astype(dtype)
    span = dt * m
    a = np.stack([rng.uniform(0.3, 0.8, B) * span, rng.uniform(0.03, 0.1, B) * span, rng.uniform(0.1, 0.4, B) * span,
                  np.geomspace(8.0, 400.0, B) * dt, np.geomspace(8.0, 400.0, B)[::-1] * dt], 1)
    return x, ic.response(m, centre=0.08, width=0.012).astype(dtype), a.astype(dtype)


def _columns(m, dtype, nontemporal):
    x, irf, a = mixed_case(m, dtype)
    bp = vp.BatchProblem(mixed_model(x, dtype), np.zeros((B, m), dtype=dtype), irf=irf)
    bp.set_column_fit(8, nontemporal)
    Phi, dPhi = bp.basis(a)
    Phi_skip, _ = bp.basis(a, skip_invariant=True, want_dphi=False)
    bp.close()
    return Phi, dPhi, Phi_skip


@pytest.mark.parametrize("dtype,m", [(np.float64, 129), (np.float64, 130), (np.float32, 257), (np.float32, 260)])
def test_columns_do_not_depend_on_the_store_kind(dtype, m):
    """fp64: m = 129 is element-wise and puts one row into the scan's second tile, m = 130 is 16-byte groups; fp32: 257 and
    260 likewise (tiles of 256 rows, groups of four)"""
    x, irf, a = mixed_case(m, dtype)
    Phi, dPhi, Phi_skip = _columns(m, dtype, 1)
    Phi_o, dPhi_o, Phi_skip_o = _columns(m, dtype, 0)
    assert Phi.dtype == dtype and Phi.shape == (B, 6, m) and dPhi.shape == (B, 5, m) and Phi_skip.shape == (B, 5, m)
    # the descriptor is the one meant: finite columns, every derivative column written, the response and the constant exact
    assert np.isfinite(Phi).all() and np.isfinite(dPhi).all() and (np.abs(dPhi).max(2) > 0).all()
    assert np.array_equal(Phi[:, 3], np.broadcast_to(irf, (B, m))) and (Phi[:, 5] == 1).all()
    assert np.array_equal(Phi_skip, Phi[:, :5])
    assert np.array_equal(Phi_o, Phi)
    assert np.array_equal(dPhi_o, dPhi)
    assert np.array_equal(Phi_skip_o, Phi_skip)


@functools.lru_cache(maxsize=None)
def _fit_data(m=129):
    """noisy data of the mixed model from numpy columns (the mirrors of tests/irf_cases.py and irf_periodic_cases.py), a box
    with a two-sided, a lower-only and an unbounded parameter, guesses 5 % off and strictly inside"""
    rng = np.random.default_rng(4300 + m)
    x = np.linspace(0.0, 12.5, m)
    dt = ic.grid_step(x)
    irf = ic.response(m, centre=0.08, width=0.012)
    truth = np.stack([rng.uniform(7.0, 9.0, B), rng.uniform(0.5, 0.8, B), rng.uniform(1.5, 2.5, B), rng.uniform(0.5, 1.0, B),
                      rng.uniform(3.5, 5.5, B)], 1)
    c = rng.uniform(0.5, 2.0, (B, 6)) * np.array([8.0, 5.0, 10.0, 3.0, 4.0, 1.0])
    Phi = np.stack([np.stack([gauss(x, t[0], t[1]), np.exp(-x / t[2]), ic.recurrence(irf, dt, t[3])[0], irf,
                              pc.mirror(irf, dt, t[4])[0], np.ones(m)]) for t in truth])
    Y = np.einsum("bnm,bn->bm", Phi, c)
    Y = Y + 1e-3 * np.abs(Y).max(1, keepdims=True) * rng.standard_normal(Y.shape)
    lo, hi = np.array([-np.inf, 0.2, 0.5, 0.2, 2.0]), np.array([np.inf, 2.0, np.inf, 3.0, 8.0])
    guess = inside(truth * (1 + rng.uniform(-0.05, 0.05, truth.shape)), lo, hi)
    for v in (x, irf, Y, lo, hi, guess):
        v.setflags(write=False)
    return x, irf, Y, lo, hi, guess


def test_a_bounded_fit_does_not_depend_on_the_store_kind():
    """the bounded variants of both kernels (element-wise at m = 129), stepped by the LM driver: parameters, coefficients and
    reports of the two store kinds are the same bits"""
    x, irf, Y, lo, hi, guess = _fit_data()
    out = []
    for nontemporal in (1, 0):
        bp = vp.BatchProblem(mixed_model(x), Y, irf=irf)
        bp.set_bounds(lo, hi)
        bp.set_column_fit(8, nontemporal)
        out.append(bp.fit(guess))
        bp.close()
    (a, C, rep), (a_o, C_o, rep_o) = out
    r = vp.BatchProblem.report_to_numpy(rep)
    print("bounded mixed fit, m=129: %d of %d converged, mean evaluations %.1f" % ((r["termination"] > 0).sum(), B, r["n_evals"].mean()))
    assert ((a >= lo) & (a <= hi)).all() and (r["n_evals"] > 1).all()
    assert np.array_equal(a_o, a) and np.array_equal(C_o, C, equal_nan=True) and report_equal(rep_o, rep)
