"""Data and the numpy checkers of the periodic IRF reconvolution tests (tests/test_irf_periodic_host.py,
tests/test_gpu_irf_periodic.py).

Convention (include/varpro_hip.h, "Periodic IRF reconvolution"): the response is zero outside the record and repeats with
period T = P dt, P >= m real; rho = exp(-dt/tau):
    Phi_i = sum_{p>=0} sum_k irf_k rho^(i-k+pP)   over the terms with i-k+pP >= 0,    dPhi_i/dtau = dt/tau^2 H_i
``periodic_sums`` is the long-double reference: per pair (i, k), with d the smallest non-negative lag (i-k, or i-k+P for
k > i), the geometric series over the periods in closed form, D = -expm1(-T/tau), E = exp(-T/tau):
    sum_p rho^(d+pP)             = rho^d / D
    sum_p (d+pP) rho^(d+pP)      = rho^d (d/D + P E/D^2)
    sum_p (d+pP)^2 rho^(d+pP)    = rho^d (d^2/D + 2 d P E/D^2 + P^2 E (1+E)/D^3)
``mirror`` is the library's numpy mirror (varpro_amd.model.irf_columns): the sequential recurrence in the dtype of the
response, a totals pass and a pass from the steady-state carry -- the reference of the device's error and the model of the
oracle's closures."""
import functools

import numpy as np

import irf_cases as ic
import varpro_amd as vp
from varpro_amd import basis
from varpro_amd.model import irf_columns

L = np.longdouble


def period_of(m, dt, period):
    """T in long double from the inputs as the library sees them (dt and period already rounded to the dtype): m dt for
    period None / 0"""
    return L(m) * L(dt) if not period else L(period)


def periodic_sums(irf, dt, tau, period=None):
    """(F, H, G, dt/tau^2) in long double, G the second-moment sum (the sensitivity of the derivative): the lags 0..m-1 of
    k <= i are a convolution, the wrapped lags P-j, j = k-i = 1..m-1, a correlation (a convolution of the reversed response)"""
    v = np.asarray(irf).astype(L)
    m = v.size
    dt, tau = L(dt), L(tau)
    T = period_of(m, dt, period)
    P = T / dt
    E, D = np.exp(-(T / tau)), -np.expm1(-(T / tau))

    def weights(d):
        r = np.exp(-(d * dt) / tau)
        return r / D, r * (d / D + P * E / D ** 2), r * (d * d / D + 2 * d * P * E / D ** 2 + P * P * E * (1 + E) / D ** 3)

    lin = weights(np.arange(m).astype(L))
    wrap = [np.concatenate([[L(0)], w]) for w in weights(P - np.arange(1, m).astype(L))]
    out = [np.convolve(v, a)[:m] + np.convolve(v[::-1], b)[:m][::-1] for a, b in zip(lin, wrap)]
    return out[0], out[1], out[2], dt / (tau * tau)


def brute_force_sums(irf, dt, tau, period=None, periods=60):
    """F and H by the defining double sum truncated after `periods` periods, long double"""
    v = np.asarray(irf).astype(L)
    m = v.size
    dt, tau = L(dt), L(tau)
    P = period_of(m, dt, period) / dt
    F, H = np.zeros(m, L), np.zeros(m, L)
    for i in range(m):
        for k in range(m):
            for p in range(periods):
                d = L(i - k) + p * P
                if d >= 0:
                    r = np.exp(-(d * dt) / tau)
                    F[i] += v[k] * r
                    H[i] += v[k] * d * r
    return F, H


def mirror(irf, dt, tau, period=None):
    """(Phi column, dPhi/dtau column) of the library's numpy mirror, periodic form (period None: one record = one period)"""
    return irf_columns(irf, dt, tau, 0.0 if period is None else period)


def column_errors(F, Dcol, irf, dt, tau, eps, period=None, sums=None):
    """irf_cases.column_errors in the sensitivity units of the periodic sums: l_i = H_i/F_i, l'_i = G_i/H_i"""
    return ic.column_errors(F, Dcol, irf, dt, tau, eps, sums if sums is not None else periodic_sums(irf, dt, tau, period))


# ---- the periodic lifetime model: c1 (irf * exp tau1) + c2 (irf * exp tau2) + c3 irf + c4, decays of the periodic kind ----
def periodic_lifetime_model(x, dtype=np.float64):
    return (vp.SeparableModelBuilder(["tau1", "tau2"], dtype=dtype)
            .function(["tau1"], basis.EXP_DECAY_IRF_PERIODIC).partial_deriv("tau1")
            .function(["tau2"], basis.EXP_DECAY_IRF_PERIODIC).partial_deriv("tau2")
            .invariant_function(basis.IRF).invariant_function(basis.CONST)
            .independent_variable(x).initial_parameters([1.0, 4.0]).build())


def periodic_lifetime_closures(x, irf, period=None):
    """the same model as numpy closures built on the numpy mirror (one evaluation per tau shared by value and derivative)"""
    x = np.asarray(x, dtype=np.float64)
    irf = np.asarray(irf, dtype=np.float64)
    dt = ic.grid_step(x)
    cached = functools.lru_cache(maxsize=8)(lambda tau: mirror(irf, dt, tau, period))
    return (vp.ClosureModel(["tau1", "tau2"], x)
            .function(["tau1"], lambda x, t: cached(float(t))[0]).partial_deriv("tau1", lambda x, t: cached(float(t))[1])
            .function(["tau2"], lambda x, t: cached(float(t))[0]).partial_deriv("tau2", lambda x, t: cached(float(t))[1])
            .invariant_function(lambda x: irf.copy())
            .invariant_function(lambda x: np.ones_like(x)))


def periodic_lifetime_columns(irf, dt, alpha, period=None):
    """(m, 4) basis matrix of the periodic lifetime model at one (tau1, tau2), fp64"""
    return np.stack([mirror(irf, dt, alpha[0], period)[0], mirror(irf, dt, alpha[1], period)[0], irf, np.ones_like(irf)], 1)


WINDOW = 12.5  # half the window of irf_cases.lifetime_data: exp(-12.5/tau2), 1.5 - 12 % of the long decay, wraps


def periodic_lifetime_data(seed, B, m, S=1, noise=1e-2, period_bins=None):
    """B problems on x = linspace(0, 12.5, m): tau1 in [0.5, 1.5], tau2 in [3, 6], guesses 10 % off; period_bins: the period
    in units of dt (None: the record is one period)"""
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, WINDOW, m)
    dt = ic.grid_step(x)
    period = None if period_bins is None else float(period_bins * dt)
    irf = ic.response(m, centre=0.08, width=0.012)
    truth = np.stack([rng.uniform(0.5, 1.5, B), rng.uniform(3.0, 6.0, B)], 1)
    shape = (B, 4) if S == 1 else (B, S, 4)
    c = rng.uniform(0.5, 2.0, shape) * np.array([10.0, 4.0, 3.0, 1.0])
    Phi = np.stack([periodic_lifetime_columns(irf, dt, truth[b], period) for b in range(B)])  # (B, m, 4)
    Y = np.einsum("bmn,bn->bm", Phi, c) if S == 1 else np.einsum("bmn,bsn->bsm", Phi, c)
    Y = Y + noise * np.abs(Y).max(-1, keepdims=True) * rng.standard_normal(Y.shape)
    guess = truth * (1 + rng.uniform(-0.1, 0.1, truth.shape))
    return dict(x=x, irf=irf, truth=truth, Y=Y, guess=guess, dt=dt, period=period)


def periodic_lifetime_costs(irf, dt, cand, Y, period=None):
    """numpy costs (B, K) of every candidate (K, 2) for a shared response, and |y|^2 (B,): lstsq on Phi, 1/2 ||r||^2"""
    cost = np.empty((Y.shape[0], cand.shape[0]))
    for k in range(cand.shape[0]):
        P = periodic_lifetime_columns(irf, dt, cand[k], period)
        r = Y.T - P @ np.linalg.lstsq(P, Y.T, rcond=None)[0]
        cost[:, k] = 0.5 * (r * r).sum(0)
    return cost, (Y * Y).sum(1)
