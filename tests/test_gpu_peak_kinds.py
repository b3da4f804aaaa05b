"""GPU tier of the peak / baseline basis kinds (VP_BASIS_GAUSS, VP_BASIS_LORENTZ, VP_BASIS_LINEAR): a descriptor that
contains one of them makes a DEVICE-COLUMN handle -- the column kernel (varpro_amd/csrc/vp_cols.hpp) evaluates Phi / dPhi
into device memory and the kernels of caller-evaluated models do everything downstream.  The checker is the oracle driven
by the closures of tests/test_gpu_external.py (the same formulas), with the contracts of K.EXTFIT / K.EVALUATION_REL_TOL;
the caller-evaluated route, fed with the columns vp_basis returns, must agree BIT FOR BIT."""
import numpy as np
import pytest

import contracts as K
import varpro_amd as vp
from oracle import oracle as O
from varpro_amd import basis
from test_gpu_external import (gauss, gauss_dmu, gauss_dsg, lorentz, lorentz_dga, lorentz_dmu, oracle_problem, peaks_data,
                               peaks_model)
from test_gpu_extfit import compare_with_oracle, oracle_fits

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def dev_peaks_model(x, dtype=np.float64):
    """`peaks_model` in the descriptor language: c1 Gauss(mu1, s1) + c2 Lorentz(mu2, g2) + c3 (n = 3, q = 4, p = 4)"""
    return (vp.SeparableModelBuilder(["mu1", "s1", "mu2", "g2"], dtype=dtype)
            .function(["mu1", "s1"], basis.GAUSS).partial_deriv("mu1").partial_deriv("s1")
            .function(["mu2", "g2"], basis.LORENTZ).partial_deriv("mu2").partial_deriv("g2")
            .invariant_function(basis.CONST)
            .independent_variable(x).initial_parameters([3.0, 0.7, 6.4, 0.9]).build())


def columns_from(dc):
    """the caller's model of an external handle: the columns a device-column handle's vp_basis returns"""
    def evaluate(alpha, want):
        return dc.basis(alpha)
    return evaluate


def report_equal(a, b):
    a, b = vp.BatchProblem.report_to_numpy(a), vp.BatchProblem.report_to_numpy(b)
    return (np.array_equal(a["termination"], b["termination"]) and np.array_equal(a["n_evals"], b["n_evals"])
            and np.array_equal(a["objective"], b["objective"], equal_nan=True))


# ---- 1. columns ------------------------------------------------------------------------------------------------------
def _longdouble_columns(x, a):
    """Phi (B, 3, m), dPhi (B, 4, m) and the exponent u (B, 1, m) of the Gaussian in np.longdouble"""
    L = np.longdouble
    xl = x.astype(L)
    mu1, s1, mu2, g2 = (a[:, k:k + 1].astype(L) for k in range(4))
    d1, d2 = xl - mu1, xl - mu2
    u = L(0.5) * (d1 / s1) ** 2
    g = np.exp(-u)
    den = d2 * d2 + g2 * g2
    Phi = np.stack([g, g2 * g2 / den, np.ones_like(g)], 1)
    dPhi = np.stack([g * d1 / s1 ** 2, g * d1 ** 2 / s1 ** 3, 2 * g2 ** 2 * d2 / den ** 2, 2 * g2 * d2 ** 2 / den ** 2], 1)
    return Phi, dPhi, u[:, None, :]


def _unit_errors(got, ref, u, eps=EPS):
    """max |got - ref| in units of eps (1 + |u|) |ref| (entries whose exact value is 0 must be 0)"""
    ref64 = ref.astype(np.float64)
    zero = ref64 == 0
    assert (np.asarray(got)[zero] == 0).all()
    scale = eps * (1 + np.abs(u).astype(np.float64)) * np.abs(ref64)
    err = np.abs(np.asarray(got).astype(np.longdouble) - ref).astype(np.float64)
    return float((err[~zero] / scale[~zero]).max())


def _column_parameters(rng, B, x):
    _t, _c, _Y, a = peaks_data(rng, B, x)
    a[B // 2:, 1] = rng.uniform(0.25, 0.4, B - B // 2)   # far tails of the Gaussian: |d| / sigma up to 30
    a[B // 2:, 3] = rng.uniform(0.02, 0.3, B - B // 2)   # ... and narrow Lorentzians
    return a


@pytest.mark.parametrize("m", [200, 1000, 10001])
@pytest.mark.parametrize("per_problem_grid", [False, True])
def test_columns_against_long_double(m, per_problem_grid):
    """vp_basis (fp64) against the same formulas in long double.  exp(-u) carries the rounding of its argument, ~|u| eps, so
    errors are measured in units of eps (1 + |u|) |value|; the bound is numpy's own error in these units, twice, plus 1"""
    rng = np.random.default_rng(31 + m)
    B = 12
    x = np.linspace(0.0, 10.0, m)
    a = _column_parameters(rng, B, x)
    X = x[None, :] + rng.uniform(-0.004, 0.004, (B, m)) if per_problem_grid else x
    dc = vp.BatchProblem(dev_peaks_model(x), np.zeros((B, m)), x=X)
    Phi, dPhi = dc.basis(a)
    dc.close()
    Xb = X if per_problem_grid else np.broadcast_to(x, (B, m))
    refs = [_longdouble_columns(Xb[b], a[b:b + 1]) for b in range(B)]
    Phi_l, dPhi_l, u = (np.concatenate([r[k] for r in refs]) for k in range(3))
    assert np.abs(u).max() > 200  # the far tails are in
    mu1, s1, mu2, g2 = (a[:, k:k + 1] for k in range(4))
    with np.errstate(all="ignore"):
        Phi_n = np.stack([gauss(Xb, mu1, s1), lorentz(Xb, mu2, g2), np.ones_like(Xb)], 1)
        dPhi_n = np.stack([gauss_dmu(Xb, mu1, s1), gauss_dsg(Xb, mu1, s1), lorentz_dmu(Xb, mu2, g2), lorentz_dga(Xb, mu2, g2)], 1)
    uP = np.concatenate([u, 0 * u, 0 * u], 1)
    uD = np.concatenate([u, u, 0 * u, 0 * u], 1)
    dev = max(_unit_errors(Phi, Phi_l, uP), _unit_errors(dPhi, dPhi_l, uD))
    ref = max(_unit_errors(Phi_n, Phi_l, uP), _unit_errors(dPhi_n, dPhi_l, uD))
    print("columns m=%d per_problem_grid=%s: device max %.3f, numpy max %.3f [eps (1+|u|) |value|]" % (m, per_problem_grid, dev, ref))
    assert dev <= 2 * ref + 1, (dev, ref)


@pytest.mark.parametrize("m", [600, 602, 1003])
def test_columns_fp32_against_long_double(m):
    """fp32 columns, 16-byte groups of four rows (m = 600) and element-wise (602, 1003), at the ROUNDED fp32 grid and parameters:
    the same rule as in fp64 -- numpy's own float32 error in units of eps32 (1 + |u|) |value|, twice, plus 1.  Values below
    the smallest normal fp32 number are left out (flush-to-zero is the device's and numpy's own business)."""
    rng = np.random.default_rng(61 + m)
    B = 8
    x32 = np.linspace(0.0, 10.0, m).astype(np.float32)
    _t, _c, _Y, a = peaks_data(rng, B, x32.astype(np.float64))
    a32 = a.astype(np.float32)
    dc = vp.BatchProblem(dev_peaks_model(x32, np.float32), np.zeros((B, m), dtype=np.float32))
    Phi, dPhi = dc.basis(a32)
    dc.close()
    assert Phi.dtype == np.float32
    Phi_l, dPhi_l, u = _longdouble_columns(x32.astype(np.float64), a32.astype(np.float64))
    Xb = np.broadcast_to(x32, (B, m))
    mu1, s1, mu2, g2 = (a32[:, k:k + 1] for k in range(4))
    Phi_n = np.stack([gauss(Xb, mu1, s1), lorentz(Xb, mu2, g2), np.ones_like(Xb)], 1)
    dPhi_n = np.stack([gauss_dmu(Xb, mu1, s1), gauss_dsg(Xb, mu1, s1), lorentz_dmu(Xb, mu2, g2), lorentz_dga(Xb, mu2, g2)], 1)
    assert Phi_n.dtype == np.float32 and dPhi_n.dtype == np.float32
    e32 = float(np.finfo(np.float32).eps)
    tiny = float(np.finfo(np.float32).tiny)

    def worst(got_P, got_D):
        out = 0.0
        for got, ref, uu in ((got_P, Phi_l, np.concatenate([u, 0 * u, 0 * u], 1)), (got_D, dPhi_l, np.concatenate([u, u, 0 * u, 0 * u], 1))):
            keep = (np.abs(ref) >= 16 * tiny) | (ref == 0)
            out = max(out, _unit_errors(np.where(keep, got, 0), np.where(keep, ref, 0), uu, eps=e32))
        return out
    dev, ref = worst(Phi, dPhi), worst(Phi_n, dPhi_n)
    print("fp32 columns m=%d: device max %.3f, numpy float32 max %.3f [eps32 (1+|u|) |value|]" % (m, dev, ref))
    assert dev <= 2 * ref + 1, (dev, ref)


def test_columns_fp32_skip_invariant_and_host_mirror():
    rng = np.random.default_rng(37)
    m, B = 602, 5  # (not a multiple of the fp32 group of 4 rows)
    x = np.linspace(0.0, 10.0, m)
    _t, _c, _Y, a = peaks_data(rng, B, x)
    Phi_l, dPhi_l, _u = _longdouble_columns(x, a)
    dc = vp.BatchProblem(dev_peaks_model(x, np.float32), np.zeros((B, m), dtype=np.float32))
    Phi, dPhi = dc.basis(a.astype(np.float32))
    assert np.abs(Phi - Phi_l).max() <= 2e-4 * np.abs(Phi_l).max()      # the fp32 legs of tests/test_gpu_external.py
    for k in range(4):
        assert np.abs(dPhi[:, k] - dPhi_l[:, k]).max() <= 2e-4 * float(np.abs(dPhi_l[:, k]).max())
    Phi2, _ = dc.basis(a.astype(np.float32), skip_invariant=True)       # VP_BASIS_CONST columns only are omitted
    assert Phi2.shape == (B, 2, m) and np.array_equal(Phi2, Phi[:, :2])
    dc.close()
    # the host mirror (SeparableModel.eval) and the device agree on a fp64 model with a linear baseline
    mdl = (vp.SeparableModelBuilder(["mu", "s"]).function(["mu", "s"], basis.GAUSS).partial_deriv("mu").partial_deriv("s")
           .invariant_function(basis.LINEAR).invariant_function().independent_variable(x).initial_parameters([3.0, 0.6]).build())
    dc = vp.BatchProblem(mdl, np.zeros((1, m)))
    Phi, dPhi = dc.basis(np.array([[3.0, 0.6]]))
    P2, _ = dc.basis(np.array([[3.0, 0.6]]), skip_invariant=True)
    dc.close()
    assert np.abs(Phi[0].T - mdl.eval()).max() <= 1e-14 and np.array_equal(Phi[0, 1], x) and (Phi[0, 2] == 1).all()
    assert P2.shape == (1, 2, m) and np.array_equal(P2[0, 1], x)       # the linear column is not a VP_BASIS_CONST column
    assert np.abs(dPhi[0, 1] - mdl.eval_partial_deriv(1)[:, 0]).max() <= 1e-14 * np.abs(dPhi[0, 1]).max()


# ---- 2. one evaluation against the oracle ------------------------------------------------------------------------------
def _evaluation_matches_oracle(cm, got, Y, alpha, w, tol=K.EVALUATION_REL_TOL):
    """the scaling of tests/test_gpu_external.py::_check_against_oracle"""
    sh = cm.shape()
    B, m = Y.shape[0], Y.shape[-1]
    S = 1 if Y.ndim == 2 else Y.shape[1]
    W = np.ones(m) if w is None else np.asarray(w)
    dPhi = cm.derivs_batch(alpha)
    assert (np.asarray(got["status"]) == 0).all()
    for b in range(B):
        p = oracle_problem(cm, Y[b], w=w)
        p.set_params(alpha[b])
        assert p.cached()
        c_ref, r_ref, J_ref = p.linear_coefficients(), p.residuals(), p.jacobian()
        yw = (Y[b] * W).reshape(-1)
        assert np.abs(np.asarray(got["C"][b]) - c_ref).max() <= tol * np.abs(c_ref).max(), "C of problem %d" % b
        assert np.abs(got["r"][b] - r_ref).max() <= tol * np.abs(yw).max(), "r of problem %d" % b
        cs = np.asarray(c_ref).reshape(S, sh.n_basis)
        for k in range(sh.n_params):
            dk = np.zeros((sh.n_basis, m))
            for pi, (j, kk) in enumerate(cm.pairs()):
                if kk == k:
                    dk[j] += dPhi[b, pi]
            unproj = max(np.abs((dk * cs[s][:, None]).sum(0) * W).max() for s in range(S))
            bound = tol * np.abs(J_ref[k]).max() + 1e-13 * unproj
            assert np.abs(got["J"][b, k] - J_ref[k]).max() <= bound, "J[%d] of problem %d" % (k, b)
        cost_ref = 0.5 * (r_ref ** 2).sum()
        assert abs(got["cost"][b] - cost_ref) <= tol * max(cost_ref, (yw ** 2).sum() * 1e-6)


@pytest.mark.parametrize("m", [200, 1000, 3000, 5000, 10001])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("S", [1, 3])
def test_one_evaluation_matches_the_oracle_and_the_caller_evaluated_route(m, weighted, S):
    rng = np.random.default_rng(7 + m + S)
    B = 4
    x = np.linspace(0.0, 10.0, m)
    cm = peaks_model(x)
    truth, _c, Y, guess = peaks_data(rng, B, x)
    if S > 1:
        C = rng.uniform(1, 30, (B, S, 3))
        Y = np.einsum("bsn,bnm->bsm", C, cm.eval_batch(truth)) + 1e-2 * rng.standard_normal((B, S, m))
    w = (0.5 + rng.random(m)) if weighted else None
    dc = vp.BatchProblem(dev_peaks_model(x), Y, weights=w)
    got = dc.evaluate(guess)
    _evaluation_matches_oracle(cm, got, Y, guess, w)
    # 3a. the same arithmetic as the caller-evaluated route: vp_basis' columns through evaluate_with_basis, bit for bit
    Phi, dPhi = dc.basis(guess)
    ext = vp.BatchProblem(cm.shape(), Y, weights=w)
    ref = ext.evaluate_with_basis(guess, Phi, dPhi)
    for key in ("r", "J", "C", "cost", "status"):
        assert np.array_equal(np.asarray(got[key]), np.asarray(ref[key])), key
    # the trait-level sequence on the device-column handle
    dc.set_params(guess)
    ext.set_params_with_basis(guess, Phi, dPhi)
    assert np.array_equal(np.asarray(dc.residuals()), np.asarray(ext.residuals()))
    assert np.array_equal(np.asarray(dc.jacobian()), np.asarray(ext.jacobian()))
    assert np.array_equal(np.asarray(dc.linear_coefficients()), np.asarray(ext.linear_coefficients()))
    assert np.array_equal(np.asarray(dc.cost()), np.asarray(ext.cost()))
    assert np.array_equal(np.asarray(dc.best_fit()), np.asarray(ext.best_fit()))
    ext.close()
    dc.close()


# ---- 3b / 4. fits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [200, 1000, 3000, 5000, 10001])
@pytest.mark.parametrize("weighted", [False, True])
def test_fit_matches_the_oracle_and_the_stepped_fit_bit_for_bit(m, weighted):
    rng = np.random.default_rng(100 + m)
    B = 48
    x = np.linspace(0.0, 10.0, m)
    cm = peaks_model(x)
    _truth, _c, Y, guess = peaks_data(rng, B, x, noise=1e-2)
    w = (0.5 + rng.random(m)) if weighted else None
    ref = oracle_fits(cm, Y, guess, w)
    dc = vp.BatchProblem(dev_peaks_model(x), Y, weights=w)
    a, C, rep = dc.fit(guess)
    compare_with_oracle(rep, a, ref)
    for b in range(0, B, 7):
        if ref[1][b] > 0:
            p = oracle_problem(cm, Y[b], w=w)
            p.set_params(a[b])
            assert np.abs(C[b] - p.linear_coefficients()).max() <= 1e-9 * np.abs(C[b]).max()
    # the handle's state is the fitted point, columns included: no further call is needed
    assert np.array_equal(np.asarray(dc.params()), a) and np.array_equal(np.asarray(dc.linear_coefficients()), C)
    r = np.asarray(dc.residuals())
    okb = rep["termination"] > 0
    assert (np.abs(0.5 * (r ** 2).sum(1) - rep["objective"])[okb] <= 1e-9 * rep["objective"][okb]).all()  # per problem
    bf = np.asarray(dc.best_fit())
    W = np.ones(m) if w is None else w
    assert np.abs((Y - bf) * W - r).max() <= 1e-9 * np.abs(Y * W).max()
    st = dc.statistics()
    assert (np.asarray(st["status"])[okb] == 0).all() and np.isfinite(np.asarray(st["cov"])[okb]).all()
    b0 = int(np.nonzero(okb)[0][0])
    p = oracle_problem(cm, Y[b0], w=w)
    p.set_params(a[b0])
    so = p.statistics()
    assert abs(st["reduced_chi2"][b0] - so["reduced_chi2"]) <= 1e-9 * so["reduced_chi2"]
    assert np.abs(st["cov"][b0] - so["cov"]).max() <= 1e-7 * np.abs(so["cov"]).max()
    # 3b. the stepped fit of an external handle, fed with vp_basis' columns at every step's trial points: the same bits,
    # whatever the interval at which either loop looks at the active count
    dc2 = vp.BatchProblem(dev_peaks_model(x), Y, weights=w)
    ext = vp.BatchProblem(cm.shape(), Y, weights=w)
    for every in (1, 3):
        a2, C2, rep2, _steps = ext.fit_with_model(columns_from(dc2), guess, check_every=every)
        assert np.array_equal(a, a2) and np.array_equal(C, C2) and report_equal(rep, rep2), every
    ext.close()
    dc2.close()
    dc.close()


def test_fit_fp32_and_device_pointers():
    import torch
    rng = np.random.default_rng(41)
    m, B = 600, 64
    x = np.linspace(0.0, 10.0, m)
    cm = peaks_model(x)
    _t, _c, Y, guess = peaks_data(rng, B, x, noise=1e-2)
    ref = oracle_fits(cm, Y, guess)
    # device-pointer handle: the same bits as the host-pointer handle
    host = vp.BatchProblem(dev_peaks_model(x), Y)
    a, C, rep = host.fit(guess)
    dev = torch.device("cuda:0")
    bp = vp.BatchProblem(dev_peaks_model(x), torch.as_tensor(Y, device=dev))
    ad, Cd, repd = bp.fit(torch.as_tensor(guess, device=dev))
    assert np.array_equal(ad.cpu().numpy(), a) and np.array_equal(Cd.cpu().numpy(), C) and report_equal(rep, repd)
    assert np.array_equal(bp.residuals().cpu().numpy(), np.asarray(host.residuals()))
    bp.close()
    host.close()
    # fp32: the minimum of the fp64 oracle at fp32 resolution
    bp = vp.BatchProblem(dev_peaks_model(x, np.float32), Y.astype(np.float32))
    a32, _C32, rep32 = bp.fit(guess.astype(np.float32))
    bp.close()
    ok = ref[1] > 0
    assert ((rep32["termination"] > 0) == ok).mean() >= 0.9
    both = ok & (rep32["termination"] > 0)
    assert np.median(np.abs(rep32["objective"] - ref[3])[both] / ref[3][both]) <= 1e-3
    assert np.median(np.abs(a32 - ref[0])[both] / np.abs(ref[0])[both]) <= 1e-3


# ---- 5. census ---------------------------------------------------------------------------------------------------------
def test_census_4096_gauss_lorentz_fits():
    """the data of test_census_4096_gauss_lorentz_fits_host_and_device_models (tests/test_gpu_extfit.py)"""
    import torch
    rng = np.random.default_rng(2024)
    m, B = 512, 4096
    x = np.linspace(0.0, 10.0, m)
    cm = peaks_model(x)
    _truth, _c, Y, guess = peaks_data(rng, B, x, noise=1e-2)
    ref = oracle_fits(cm, Y, guess)
    assert (ref[1] > 0).mean() >= 0.99  # the comparison cannot pass on a batch of failures
    dev = torch.device("cuda:0")
    bp = vp.BatchProblem(dev_peaks_model(x), torch.as_tensor(Y, device=dev))
    a, _C, rep = bp.fit(torch.as_tensor(guess, device=dev))
    s = compare_with_oracle(rep, a.cpu().numpy(), ref)
    bp.close()
    print("census device-column fit: %s" % (s,))


# ---- 6. mixed model ----------------------------------------------------------------------------------------------------
def test_mixed_model_gauss_exponential_tail_linear_baseline():
    """GAUSS(mu, s) + EXP_DECAY(tau) + LINEAR + CONST: n = 4, q = 3 -- a peak kind next to an older kind.
    The K.EXTFIT contract (objective to 1e-6) presupposes a well-posed problem: an exponential with tau of the order of the
    window is nearly a combination of the linear and the constant column (cond(Phi) ~ 5e11 on a fit that wanders there), and
    eps cond(Phi) then exceeds the contract for ANY route.  The tail therefore decays well inside the window (tau <= 1.5 of
    10) and the peak sits beyond it; the test asserts that precondition on the checker's side -- cond(Phi) < 1e3 at the
    truth and at the oracle's fitted points, no oracle fit beyond 30 evaluations -- before it compares."""
    rng = np.random.default_rng(43)
    m, B = 700, 24
    x = np.linspace(0.0, 10.0, m)
    decay = lambda x, t: np.exp(-x / t)
    cm = (vp.ClosureModel(["mu", "s", "tau"], x)
          .function(["mu", "s"], gauss).partial_deriv("mu", gauss_dmu).partial_deriv("s", gauss_dsg)
          .function(["tau"], decay).partial_deriv("tau", lambda x, t: np.exp(-x / t) * x / t ** 2)
          .invariant_function(lambda x: x.copy())
          .invariant_function(lambda x: np.ones_like(x)))
    mdl = (vp.SeparableModelBuilder(["mu", "s", "tau"])
           .function(["mu", "s"], basis.GAUSS).partial_deriv("mu").partial_deriv("s")
           .function(["tau"], basis.EXP_DECAY).partial_deriv("tau")
           .invariant_function(basis.LINEAR).invariant_function(basis.CONST)
           .independent_variable(x).initial_parameters([5.0, 0.7, 2.0]).build())
    truth = np.stack([rng.uniform(5.5, 7.5, B), rng.uniform(0.4, 0.9, B), rng.uniform(0.5, 1.5, B)], 1)
    c = np.stack([rng.uniform(5, 50, B), rng.uniform(5, 50, B), rng.uniform(-1, 1, B), rng.uniform(0, 5, B)], 1)
    Y = np.einsum("bn,bnm->bm", c, cm.eval_batch(truth))
    Y = Y + 1e-2 * np.abs(Y).max(1, keepdims=True) * rng.standard_normal(Y.shape)
    guess = truth * (1 + rng.uniform(-0.1, 0.1, truth.shape))
    dc = vp.BatchProblem(mdl, Y)
    _evaluation_matches_oracle(cm, dc.evaluate(guess), Y, guess, None)
    ref = oracle_fits(cm, Y, guess)
    assert (ref[1] > 0).all() and ref[2].max() <= 30
    assert max(np.linalg.cond(P.T) for P in np.concatenate([cm.eval_batch(truth), cm.eval_batch(ref[0])])) < 1e3
    a, _C, rep = dc.fit(guess)
    compare_with_oracle(rep, a, ref)
    dc.close()


# ---- 7. global fits ------------------------------------------------------------------------------------------------------
def test_global_fit_of_17_right_hand_sides_and_its_statistics():
    """the tolerances of tests/test_gpu_extfit.py::test_several_right_hand_sides"""
    S = 17
    rng = np.random.default_rng(50 + S)
    B, m = 12, 400
    x = np.linspace(0.0, 10.0, m)
    cm = peaks_model(x)
    truth, _c, _Y1, guess = peaks_data(rng, B, x, noise=1e-2)
    Phi = cm.eval_batch(truth)
    Cs = np.stack([rng.uniform(5, 50, (B, S)), rng.uniform(5, 50, (B, S)), rng.uniform(0, 5, (B, S))], 2)
    Y = np.einsum("bsn,bnm->bsm", Cs, Phi)
    Y = Y + 1e-2 * np.abs(Y).max(2, keepdims=True) * rng.standard_normal(Y.shape)
    dc = vp.BatchProblem(dev_peaks_model(x), Y)
    a1, C1, rep1 = dc.fit(guess)
    rep = vp.BatchProblem.report_to_numpy(rep1)
    assert np.asarray(C1).shape == (B, S, 3)
    for b in range(B):
        p = oracle_problem(cm, Y[b])
        p.set_params(guess[b])
        r = p.fit()
        assert (rep["termination"][b] > 0) == (r.termination > 0), (b, rep[b], r.termination)
        if r.termination > 0:
            assert abs(rep["objective"][b] - r.objective) <= 1e-6 * r.objective, (b, rep["objective"][b], r.objective)
            assert abs(int(rep["n_evals"][b]) - int(r.n_evals)) <= 4
            a_ref = p.params()
            assert np.abs(np.asarray(a1)[b] - a_ref).max() <= 1e-5 * np.abs(a_ref).max()
            Cr = np.asarray(p.linear_coefficients()).reshape(S, 3)
            assert np.abs(np.asarray(C1)[b] - Cr).max() <= 1e-5 * np.abs(Cr).max()
    # global statistics right after the fit: no further call is needed
    g0 = dc.global_statistics(want_confidence_sigma=True)
    assert (np.asarray(g0["status"]) == 0).all() and np.isfinite(np.asarray(g0["cov_alpha"])).all()
    # ... and bit-identical to the external-handle route given the same columns AND the same cached state: an external
    # handle gets its coefficients from set_params_with_basis (a fit's come from the step kernel and differ in the last
    # bits), so the device-column handle takes the same call, vp_set_params, at the fitted point
    dc.set_params(a1)
    gs = dc.global_statistics(want_confidence_sigma=True)
    assert np.allclose(np.asarray(g0["cov_alpha"]), np.asarray(gs["cov_alpha"]), rtol=1e-6, atol=0)
    Phi_f, dPhi_f = dc.basis(a1)
    ext = vp.BatchProblem(cm.shape(), Y)
    ext.set_params_with_basis(a1, Phi_f, dPhi_f)
    ge = ext.global_statistics(want_confidence_sigma=True)
    for key in ("cov_alpha", "reduced_chi2", "coef_cov", "coef_alpha_cov", "conf_sigma", "status"):
        assert np.array_equal(np.asarray(gs[key]), np.asarray(ge[key]), equal_nan=(key != "status")), key
    assert (np.asarray(gs["status"]) == 0).all()
    ext.close()
    dc.close()


# ---- 8. handle reuse and throughput mode -------------------------------------------------------------------------------
def test_set_observations_and_fit_pipeline():
    import torch
    rng = np.random.default_rng(47)
    m, B = 512, 256
    x = np.linspace(0.0, 10.0, m)
    mdl = dev_peaks_model(x)
    batches = [peaks_data(rng, B, x, noise=1e-2) for _ in range(4)]
    fresh = []
    for _t, _c, Y, g in batches:
        bp = vp.BatchProblem(mdl, Y)
        fresh.append(bp.fit(g))
        bp.close()
    bp = vp.BatchProblem(mdl, batches[0][2])
    bp.fit(batches[0][3])
    bp.set_observations(batches[1][2])
    with pytest.raises(vp.VarproHipError):
        bp.cost()  # the cached fit belonged to the old data
    a, C, rep = bp.fit(batches[1][3])
    assert np.array_equal(a, fresh[1][0]) and np.array_equal(C, fresh[1][1]) and report_equal(rep, fresh[1][2])
    bp.close()
    dev = torch.device("cuda:0")
    pipe = vp.FitPipeline(mdl, torch.as_tensor(batches[0][2], device=dev), n_slots=2)
    outs = [pipe.submit(torch.as_tensor(Y, device=dev), torch.as_tensor(g, device=dev)) for _t, _c, Y, g in batches]
    pipe.wait()
    torch.cuda.synchronize()
    for (a, C, rep, _slot), f in zip(outs, fresh):
        assert np.array_equal(a.cpu().numpy(), f[0]) and np.array_equal(C.cpu().numpy(), f[1]) and report_equal(rep, f[2])
    pipe.close()


# ---- 9. degenerate parameters --------------------------------------------------------------------------------------------
def test_degenerate_parameters_are_latched_per_problem():
    """sigma = 0, gamma = 0 and a NaN guess.  What the formulas give there, for the closures as for the device: with the peak
    centre ON a grid point the value is 0 / 0 -- a non-finite Phi, residuals() == None, a non-zero status; with the centre
    between grid points a width of 0 gives a FINITE Phi (exp(-inf) = 0, 0 / d^2 = 0) and, for the Gaussian, NaN derivatives
    (0 * d / 0): status 0 and a fit that ends `Numerical` at its first Jacobian.  Every such problem ends with the oracle's
    termination code; its status is non-zero wherever the closures' Phi is not finite and everywhere equals the status the
    caller-evaluated route latches for the closures' own columns.  The batch is never aborted."""
    from test_gpu_extfit import host_model
    rng = np.random.default_rng(53)
    m, B = 300, 32
    x = np.linspace(0.0, 10.0, m)
    cm = peaks_model(x)
    _t, _c, Y, guess = peaks_data(rng, B, x, noise=1e-2)
    bad = guess.copy()
    bad[3, :2] = x[90], 0.0     # sigma = 0, centre on a grid point
    bad[5, 1] = 0.0             # sigma = 0, centre between grid points
    bad[11, 3] = 0.0            # gamma = 0, centre between grid points
    bad[13, 2:] = x[200], 0.0   # gamma = 0, centre on a grid point
    bad[20, 0] = np.nan         # a NaN guess
    idx = [3, 5, 11, 13, 20]
    good = np.setdiff1d(np.arange(B), idx)
    with np.errstate(all="ignore"):
        phi_finite = np.isfinite(cm.eval_batch(bad)).all((1, 2))
        Phi_c, dPhi_c = cm.eval_batch(bad), cm.derivs_batch(bad)
    assert list(np.nonzero(~phi_finite)[0]) == [3, 13, 20]
    dc = vp.BatchProblem(dev_peaks_model(x), Y)
    ext = vp.BatchProblem(cm.shape(), Y)
    ev = dc.evaluate(bad)
    ev_ext = ext.evaluate_with_basis(bad, Phi_c, dPhi_c)
    assert (np.asarray(ev["status"])[~phi_finite] != 0).all() and (np.asarray(ev["status"])[good] == 0).all()
    assert np.array_equal(np.asarray(ev["status"]), np.asarray(ev_ext["status"]))
    a, C, rep = dc.fit(bad)
    with np.errstate(all="ignore"):
        _a, _C, rep_ext, _steps = ext.fit_with_model(host_model(cm), bad)
    st = np.asarray(dc.status())
    assert (st[~phi_finite] != 0).all() and (st[good] == 0).all()
    assert np.array_equal(st, np.asarray(ext.status()))
    assert np.array_equal(rep["termination"][idx], rep_ext["termination"][idx])
    with np.errstate(all="ignore"):
        for b in idx:
            p = oracle_problem(cm, Y[b])
            p.set_params(bad[b])
            assert rep["termination"][b] == p.fit().termination, (b, rep[b])
    ext.close()
    dc.close()
    # every other problem is unaffected: bit-identical to the same batch without the degenerate ones
    dc = vp.BatchProblem(dev_peaks_model(x), Y[good])
    a2, C2, rep2 = dc.fit(guess[good])
    dc.close()
    assert np.array_equal(a[good], a2) and np.array_equal(C[good], C2) and report_equal(rep[good], rep2)


# ---- 10. refusals --------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    rng = np.random.default_rng(59)
    m, B = 200, 4
    x = np.linspace(0.0, 10.0, m)
    _t, _c, Y, guess = peaks_data(rng, B, x)
    dc = vp.BatchProblem(dev_peaks_model(x), Y)
    Phi, dPhi = dc.basis(guess)
    calls = [lambda: dc.set_params_with_basis(guess, Phi, dPhi), lambda: dc.evaluate_with_basis(guess, Phi, dPhi),
             lambda: dc.jacobian_with_derivatives(dPhi), lambda: dc.fit_begin(guess),
             lambda: dc.fit_active_set(), lambda: dc.fit_end(), lambda: dc.fit_trace(guess)]
    for i, call in enumerate(calls):
        with pytest.raises(vp.VarproHipError) as e:
            call()
        assert e.value.code == -2, i  # VP_ERR_UNSUPPORTED
    dc._xf_trial, dc._xf_want = dc._empty((B, 4)), dc._empty((B,), np.int32)
    with pytest.raises(vp.VarproHipError) as e:
        dc.fit_step_with_basis(Phi, dPhi)
    assert e.value.code == -2
    dc.set_fit_kernel("slots")  # accepted, no effect
    a, _C, rep = dc.fit(guess)
    assert (rep["termination"] > 0).all()
    dc.close()
    # right-hand-side sharding, as on caller-evaluated handles
    import ctypes
    from varpro_amd import _lib
    dc = vp.BatchProblem(dev_peaks_model(x), np.stack([Y, Y], 1))
    cb = _lib.ALLREDUCE_FN(lambda ptr, count, stream, user: 0)
    assert dc.lib.vp_set_rhs_allreduce(dc._h, cb, None, 4) == -2
    assert np.isfinite(np.asarray(dc.evaluate(guess)["cost"])).all()
    dc.close()
    _ = ctypes
    # m < n: evaluations work (minimum-norm coefficients), the fit is refused like the stepped fit
    x2 = np.array([3.0, 6.5])
    dc = vp.BatchProblem(dev_peaks_model(x2), rng.uniform(1, 5, (2, 2)))
    ev = dc.evaluate(guess[:2])
    assert np.abs(np.asarray(ev["r"])).max() <= 1e-10 * 5
    with pytest.raises(vp.VarproHipError) as e:
        dc.fit(guess[:2])
    assert e.value.code == -2
    dc.close()
    # flags that select in-register kernels are accepted and have no effect
    dc = vp.BatchProblem(dev_peaks_model(x), Y, grid_recurrence=False, stream_rows=True)
    dc2 = vp.BatchProblem(dev_peaks_model(x), Y)
    assert np.array_equal(np.asarray(dc.evaluate(guess)["r"]), np.asarray(dc2.evaluate(guess)["r"]))
    dc.close()
    dc2.close()


def test_old_kinds_take_the_in_register_kernels():
    """a descriptor of the five older kinds is not a device-column handle: the caller-evaluated entries tell"""
    x = np.linspace(0.0, 10.0, 64)
    bp = vp.BatchProblem(vp.multi_exponential_model(x, [1.0, 3.0]), np.ones((2, 64)), x=x)
    with pytest.raises(vp.VarproHipError) as e:
        bp.set_params_with_basis(np.ones((2, 2)), np.ones((2, 3, 64)))
    assert "vp_batch_create_external" in str(e.value)
    a, tr = bp.fit_trace(np.tile([1.0, 3.0], (2, 1)))[0::3]
    assert np.isfinite(a).all() and np.isfinite(tr[:, 0, :2]).all()
    bp.close()
