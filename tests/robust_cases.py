"""Data, the numpy mirror and the CPU iterated fit of the robust-fit tests (tests/test_robust_host.py,
tests/test_gpu_robust.py).

``reweight_mirror`` is vp_robust_reweight in numpy, every operation in the handle's dtype and the median taken from
``np.sort``; ``rho_mirror`` is the sum of rho in long double with the sum of absolute terms its error bound is stated in.
The workloads are the two of tests/poisson_cases.py at peak counts of 300 to 3000 with 5 % of the bins spiked by 5 to 15
standard deviations; the base weights are the Neyman weights of the contaminated counts, which make the clean residuals
homoscedastic.  ``iterated_fit`` is ``BatchProblem.fit_robust`` with every round an oracle fit at the mirror's weights."""
import numpy as np

import poisson_cases as pc

L = np.longdouble
K95 = {"huber": 1.345, "cauchy": 2.385, "tukey": 4.685}
MAD_TO_SIGMA = 1.482602218505602


# ---- the mirror of the re-weighting ------------------------------------------------------------------------------------
def scale_mirror(e, w0, dtype):
    """per problem s = T(1.4826..) * T(0.5) * (a[(me-1)//2] + a[me//2]) of the sorted |e| over the me rows with w0 != 0; 0
    for me == 0; NaN where a residual of the problem (any row) is not finite"""
    T = np.dtype(dtype).type
    s = np.empty(e.shape[0], dtype)
    for b in range(e.shape[0]):
        if not np.isfinite(e[b]).all():
            s[b] = np.nan
            continue
        a = np.sort(np.abs(e[b][w0[b] != 0]))
        me = a.size
        with np.errstate(all="ignore"):
            s[b] = T(MAD_TO_SIGMA) * (T(0.5) * (a[(me - 1) // 2] + a[me // 2])) if me else T(0)
    return s


def sqrt_omega(u, loss, k, dtype):
    """sqrt(omega) of u = |e|/s >= 0 in ``dtype``, the comparisons written so that a NaN goes through"""
    T = np.dtype(dtype).type
    k = T(k)
    with np.errstate(all="ignore"):
        if loss == "huber":
            return np.where(u <= k, T(1), np.sqrt(k / u)).astype(dtype)
        t = (u / k).astype(dtype)
        if loss == "cauchy":
            return np.sqrt(T(1) / (T(1) + t * t)).astype(dtype)
        assert loss == "tukey"
        return np.where(t >= T(1), T(0), (T(1) - t) * (T(1) + t)).astype(dtype)


def reweight_mirror(Y, F, w0, loss, k, scale, dtype=np.float64):
    """(w, Y_w, s, u) as the kernel forms them: e = w0 (y - f), s = ``scale`` rounded to dtype or (scale == 0) the
    normalised median per problem, u = |e|/s, w = w0 sqrt(omega), Y_w = w y; a problem with s == 0 (estimated) keeps
    w = w0 and has u = 0; a residual that is not finite gives NaN"""
    T = np.dtype(dtype).type
    y, f = np.asarray(Y, dtype=dtype), np.asarray(F, dtype=dtype)
    w0 = np.ones_like(y) if w0 is None else np.asarray(w0, dtype=dtype)
    with np.errstate(all="ignore"):
        e = (w0 * (y - f).astype(dtype)).astype(dtype)
        a = np.abs(e)
        s = scale_mirror(e, w0, dtype) if scale == 0 else np.full(y.shape[0], T(scale), dtype)
        flat = s == 0
        u = (a / np.where(flat, T(1), s)[:, None]).astype(dtype)
        sw = sqrt_omega(u, loss, k, dtype)
        sw = np.where(np.isfinite(a), sw, T(np.nan))
        u = np.where(np.isfinite(a), u, T(np.nan))
        sw[flat], u[flat] = T(1), T(0)
        w = (w0 * sw).astype(dtype)
        yw = (w * y).astype(dtype)
    return w, yw, s, u


def rho_mirror(u, loss, k, dtype=np.float64):
    """per problem in long double from u and k rounded to ``dtype``: sum rho(u), and the sum of the absolute values of the
    terms rho is formed from (the unit of the bound on the device's fp64 sum)"""
    k = L(np.dtype(dtype).type(k))
    u = np.asarray(u, dtype=dtype).astype(L)
    with np.errstate(all="ignore"):
        if loss == "huber":
            rho = np.where(u <= k, u * u / 2, k * u - k * k / 2)
            mag = np.where(u <= k, u * u / 2, k * u + k * k / 2)
        elif loss == "cauchy":
            t = u / k
            rho = k * k / 2 * np.log1p(t * t)
            mag = rho
        else:
            t = u / k
            q = 1 - t * t
            rho = np.where(t >= 1, k * k / 6, k * k / 6 * (1 - q * q * q))
            mag = np.where(t >= 1, k * k / 6, k * k / 6 * (1 + np.abs(q * q * q)))
        rho = np.where(np.isnan(u), L(np.nan), rho)
    return rho.sum(-1), mag.sum(-1)


def rho_bound(m, vw):
    """|device rho - exact rho| <= rho_bound * eps64 * (sum of absolute terms), derived like poisson_cases.sum_bound, u the
    unit roundoff eps/2.  A term, from the same u and k in fp64 -- Huber: product, product, halving is exact: 2u of u^2/2, or
    product, product, difference: 2u (k u + k^2/2).  Cauchy: quotient, square, log1p (good to 1 ulp = 2u; the two roundings
    of its argument x move log1p by at most 2u x/(1 + x) <= 2u log1p(x)), square of k, product: 7u.  Tukey: quotient u,
    square 2u more, q = 1 - t^2 absolute 3u + u, its cube 3 (4u) + 2u relative to 1 or |q|^3, the difference u, k^2/6 and the
    product 3u: at most 20u of k^2/6 (1 + |q|^3).  The sum: a lane adds its ceil(m / (64 vw)) terms in order, six tree levels
    follow: (tiles + 6) u.  In units of eps = 2u: (20 + tiles + 6) / 2."""
    tiles = -(-m // (64 * vw))
    return (20 + tiles + 6) / 2.0


# ---- the contaminated workloads ------------------------------------------------------------------------------------------
PEAK = (300.0, 3000.0)
SPIKE_SEED, SPIKE_SHARE, SPIKE_SIGMAS = 5, 0.05, (5.0, 15.0)


def contaminate(wl):
    """spikes of 5 .. 15 standard deviations of the bin on 5 % of the bins, the sums rounded to integers; ``wl.clean`` keeps
    the counts as drawn, ``wl.spiked`` marks the bins, ``wl.w0`` are the Neyman weights of what was measured"""
    rng = np.random.default_rng(SPIKE_SEED)
    wl.clean = wl.Y
    wl.spiked = rng.random(wl.Y.shape) < SPIKE_SHARE
    height = rng.uniform(SPIKE_SIGMAS[0], SPIKE_SIGMAS[1], wl.Y.shape) * np.sqrt(np.maximum(wl.mean, 1.0))
    wl.Y = np.rint(wl.clean + np.where(wl.spiked, height, 0.0))  # (the oracle closures read wl.Y when they are called)
    wl.w0 = pc.reweight_mirror(wl.Y, None)[0]
    return wl


def workload(name):
    if name == "double_exp":
        return contaminate(pc.double_exp(pc.DOUBLE_EXP_SEED, pc.B_FIT, peak=PEAK))
    assert name == "lifetime"
    return contaminate(pc.lifetime(pc.LIFETIME_SEED, pc.B_FIT, peak=PEAK))


def iterated_fit(wl, loss, rounds, k=None):
    """BatchProblem.fit_robust on the CPU: a fit at the base weights from the guess, then ``rounds`` fits at the mirror's
    weights of the previous fit, each from the previous parameters.  Returns the list of (alpha, C, termination) after every
    fit (rounds + 1 entries) -- the convergence sequence"""
    k = K95[loss] if k is None else k
    W, seq, a = wl.w0, [], wl.guess
    for _ in range(rounds + 1):
        a, C, term, _nev, _obj = pc.oracle_round(wl, W, a)
        seq.append((a, C, term))
        W = reweight_mirror(wl.Y, pc.best_fit(wl, a, C), wl.w0, loss, k, 0.0)[0]
    return seq


def normalised_score(wl, alpha, C, loss, k=None):
    """per problem max_k |sum_i psi(u_i) g_ik| / sqrt(sum_i g_ik^2), g = w0 [Phi, c dPhi], psi = u omega(u), u = w0 (y - f)/s
    with s the normalised median of |w0 (y - f)|: each component of the estimating equations in units of the standard
    deviation it has for residuals of unit variance"""
    k = K95[loss] if k is None else k
    out = np.empty(alpha.shape[0])
    for b in range(alpha.shape[0]):
        Phi, dPhi = wl.columns(np.asarray(alpha[b], dtype=np.float64))
        c = np.asarray(C[b], dtype=np.float64)
        e = wl.w0[b] * (wl.Y[b] - Phi @ c)
        s = scale_mirror(e[None], wl.w0[b][None], np.float64)[0]
        u = e / s
        psi = u * sqrt_omega(np.abs(u), loss, k, np.float64) ** 2
        G = wl.w0[b][:, None] * np.concatenate([Phi, dPhi * c[:wl.q][None, :]], 1)
        out[b] = (np.abs(psi @ G) / np.sqrt((G * G).sum(0))).max()
    return out


def parameter_error(wl, alpha):
    """median over the batch of the largest relative error of a nonlinear parameter"""
    return float(np.median((np.abs(alpha - wl.truth) / wl.truth).max(1)))
