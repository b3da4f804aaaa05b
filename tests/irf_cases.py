"""Data and the numpy checkers of the IRF reconvolution tests (tests/test_irf_host.py, tests/test_gpu_irf.py).

Convention (include/varpro_hip.h): on a uniform grid of step dt, rho = exp(-dt/tau),
    Phi_i       = sum_{k<=i} irf_k rho^(i-k)                        F_i = irf_i + rho F_{i-1}
    dPhi_i/dtau = dt/tau^2 H_i,  H_i = sum_k (i-k) rho^(i-k) irf_k  H_i = rho (H_{i-1} + F_{i-1})
``recurrence`` is the plain sequential recurrence in the dtype of its input -- the reference of the GPU tests and the model
of the oracle's closures; ``direct_sums`` evaluates the defining sums in np.longdouble."""
import functools

import numpy as np

import varpro_amd as vp
from varpro_amd import basis

L = np.longdouble


def grid_step(x):
    """dt as the library forms it, in the dtype of x: (x[m-1] - x[0]) / (m-1); m == 1: 0"""
    x = np.asarray(x)
    T = x.dtype.type
    return T(0) if x.size == 1 else (x[-1] - x[0]) / T(x.size - 1)


def recurrence(irf, dt, tau):
    """(F, H, dt/tau^2 H) by the sequential recurrence, every operation rounded to the dtype of irf (fp64: Python floats,
    which are IEEE doubles; fp32: numpy scalars)"""
    irf = np.asarray(irf)
    T = irf.dtype.type
    m = irf.size
    if irf.dtype == np.float64:
        dt, tau = float(dt), float(tau)
        rho = float(np.exp(-(dt / tau)))
        f = h = 0.0
        F, H = [0.0] * m, [0.0] * m
        for i, v in enumerate(irf.tolist()):
            h = rho * (h + f)
            f = v + rho * f
            F[i], H[i] = f, h
        F, H = np.array(F), np.array(H)
    else:
        dt, tau = T(dt), T(tau)
        rho = np.exp(-(dt / tau))
        assert rho.dtype == irf.dtype
        f = h = T(0)
        F, H = np.empty(m, irf.dtype), np.empty(m, irf.dtype)
        for i in range(m):
            h = rho * (h + f)
            f = irf[i] + rho * f
            F[i], H[i] = f, h
    scale = T(dt) / (T(tau) * T(tau))
    return F, H, scale * H


def direct_sums(irf, dt, tau):
    """the defining sums in long double, O(m^2) (np.convolve keeps long double): F, H, G = sum_k (i-k)^2 rho^(i-k) irf_k and dt/tau^2; rho = exp(-dt/tau) is
    taken in long double from the given (already rounded) inputs"""
    v = np.asarray(irf).astype(L)
    m = v.size
    dt, tau = L(dt), L(tau)
    rho = np.exp(-(dt / tau))
    lag = np.arange(m).astype(L)
    p = rho ** lag  # rho^(i-k) by lag; the three sums are convolutions of the response with p, lag p, lag^2 p
    return (np.convolve(v, p)[:m], np.convolve(v, lag * p)[:m], np.convolve(v, lag * lag * p)[:m], dt / (tau * tau))


def unit_errors(got, ref, sens, eps):
    """max |got - ref| in units of eps (1 + sens) |ref|; entries whose exact value is 0 must be 0"""
    got = np.asarray(got)
    zero = ref == 0
    assert (got[zero] == 0).all()
    if zero.all():
        return 0.0
    err = np.abs(got.astype(L) - ref)
    scale = L(eps) * (1 + sens) * np.abs(ref)
    return float((err[~zero] / scale[~zero]).max())


def column_errors(F, D, irf, dt, tau, eps, sums=None):
    """errors of a value column F and a derivative column D in the sensitivity units of the recurrence: for Phi
    eps (1 + l_i) |Phi_i| with l_i = H_i / F_i (the relative change of F_i per relative change of rho), for the derivative
    eps (1 + l'_i) |value| with l'_i = G_i / H_i -- all references in long double (sums: a direct_sums result to reuse)"""
    Fl, Hl, Gl, sc = sums if sums is not None else direct_sums(irf, dt, tau)
    with np.errstate(all="ignore"):
        lF = np.where(Fl != 0, Hl / np.where(Fl != 0, Fl, 1), 0)
        lH = np.where(Hl != 0, Gl / np.where(Hl != 0, Hl, 1), 0)
    return unit_errors(F, Fl, lF, eps), unit_errors(D, sc * Hl, lH, eps)


def response(m, centre=0.12, width=0.015, floor=1e-3, amplitude=1.0):
    """a non-negative instrument response: a narrow Gaussian (centre and width as fractions of the window, at least 1.5
    samples wide) plus a small positive floor"""
    i = np.arange(m, dtype=np.float64)
    s = max(1.5, width * m)
    return amplitude * np.exp(-0.5 * ((i - centre * m) / s) ** 2) + floor


# ---- the lifetime model: c1 (irf * exp tau1) + c2 (irf * exp tau2) + c3 irf + c4  (n = 4, q = 2, p = 2) ------------------
def lifetime_model(x, dtype=np.float64):
    return (vp.SeparableModelBuilder(["tau1", "tau2"], dtype=dtype)
            .function(["tau1"], basis.EXP_DECAY_IRF).partial_deriv("tau1")
            .function(["tau2"], basis.EXP_DECAY_IRF).partial_deriv("tau2")
            .invariant_function(basis.IRF).invariant_function(basis.CONST)
            .independent_variable(x).initial_parameters([1.0, 4.0]).build())


def lifetime_closures(x, irf):
    """the same model as numpy closures built on ``recurrence`` (one evaluation per tau is shared by value and derivative)"""
    x = np.asarray(x, dtype=np.float64)
    irf = np.asarray(irf, dtype=np.float64)
    dt = grid_step(x)
    cached = functools.lru_cache(maxsize=8)(lambda tau: recurrence(irf, dt, tau))
    return (vp.ClosureModel(["tau1", "tau2"], x)
            .function(["tau1"], lambda x, t: cached(float(t))[0]).partial_deriv("tau1", lambda x, t: cached(float(t))[2])
            .function(["tau2"], lambda x, t: cached(float(t))[0]).partial_deriv("tau2", lambda x, t: cached(float(t))[2])
            .invariant_function(lambda x: irf.copy())
            .invariant_function(lambda x: np.ones_like(x)))


def lifetime_columns(irf, dt, alpha):
    """(m, 4) basis matrix of the lifetime model at one (tau1, tau2), fp64"""
    return np.stack([recurrence(irf, dt, alpha[0])[0], recurrence(irf, dt, alpha[1])[0], irf, np.ones_like(irf)], 1)


WINDOW = 25.0  # tau2 <= 6 decays well inside the window: the offset column stays distinguishable


def lifetime_data(seed, B, m, S=1, noise=1e-2, irf_per_problem=False):
    """B problems on x = linspace(0, 25, m): separated lifetimes tau1 in [0.5, 1.5], tau2 in [3, 6], guesses 10 % off"""
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, WINDOW, m)
    dt = grid_step(x)
    if irf_per_problem:
        irf = np.stack([response(m, centre=c, width=w) for c, w in zip(rng.uniform(0.06, 0.12, B), rng.uniform(0.008, 0.016, B))])
    else:
        irf = response(m, centre=0.08, width=0.012)
    truth = np.stack([rng.uniform(0.5, 1.5, B), rng.uniform(3.0, 6.0, B)], 1)
    shape = (B, 4) if S == 1 else (B, S, 4)
    c = rng.uniform(0.5, 2.0, shape) * np.array([10.0, 4.0, 3.0, 1.0])
    Phi = np.stack([lifetime_columns(irf[b] if irf_per_problem else irf, dt, truth[b]) for b in range(B)])  # (B, m, 4)
    Y = np.einsum("bmn,bn->bm", Phi, c) if S == 1 else np.einsum("bmn,bsn->bsm", Phi, c)
    Y = Y + noise * np.abs(Y).max(-1, keepdims=True) * rng.standard_normal(Y.shape)
    guess = truth * (1 + rng.uniform(-0.1, 0.1, truth.shape))
    return dict(x=x, irf=irf, truth=truth, Y=Y, guess=guess, dt=dt)


def lifetime_costs(irf, dt, cand, Y):
    """numpy costs (B, K) of every candidate (K, 2) of every problem, and |y|^2 (B,): lstsq on Phi, 1/2 ||r||^2.
    irf (m,) or (B, m)"""
    B, m = Y.shape
    K = cand.shape[0]
    cost = np.empty((B, K))
    for b in range(B if irf.ndim == 2 else 1):
        v = irf[b] if irf.ndim == 2 else irf
        for k in range(K):
            P = lifetime_columns(v, dt, cand[k])
            rhs = (Y[b:b + 1] if irf.ndim == 2 else Y).T
            r = rhs - P @ np.linalg.lstsq(P, rhs, rcond=None)[0]
            if irf.ndim == 2:
                cost[b, k] = 0.5 * (r * r).sum()
            else:
                cost[:, k] = 0.5 * (r * r).sum(0)
    return cost, (Y * Y).sum(1)
