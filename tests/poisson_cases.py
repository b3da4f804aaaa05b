"""Data, the numpy mirror and the CPU iterated fit of the Poisson-weighting tests (tests/test_poisson_host.py,
tests/test_gpu_poisson.py).

Counts are drawn with ``rng.poisson`` from two models: the double exponential plus offset (kinds 1, 1, 0: the in-register
kernels; the oracle fits the descriptor directly) and the lifetime model of tests/irf_cases.py (IRF reconvolution: a
device-column handle; the oracle is driven by the same closures).  Peak counts run from about 30 to about 300: the tails hold
empty bins and the fits dip under the floor of 1 there.

``reweight_mirror`` is vp_poisson_reweight in numpy: w and Y_w in the handle's dtype, the deviance and Pearson's X^2 in long
double.  ``iterated_fit`` is ``BatchProblem.fit_poisson`` with every round an oracle fit at the current weights."""
import numpy as np

import irf_cases as ic
import varpro_amd as vp
from oracle import oracle as O

L = np.longdouble
FLOOR = 1.0


# ---- the mirror of the re-weighting ------------------------------------------------------------------------------------
def reweight_mirror(Y, F=None, floor=FLOOR, dtype=np.float64):
    """(w, Y_w) in ``dtype`` as the kernel forms them -- v = x < floor ? floor : x (a NaN stays), w = 1/sqrt(v) by the IEEE
    square root and division, NaN where v is not finite, Y_w = w y -- with x = Y (F is None: Neyman) or x = F (model)"""
    T = np.dtype(dtype).type
    y = np.asarray(Y, dtype=dtype)
    x = y if F is None else np.asarray(F, dtype=dtype)
    with np.errstate(all="ignore"):
        v = np.where(x < T(floor), T(floor), x)
        w = (T(1) / np.sqrt(v)).astype(dtype)
        w = np.where(np.isfinite(v), w, T(np.nan)).astype(dtype)
        yw = (w * y).astype(dtype)
    return w, yw


def goodness_mirror(Y, F, floor=FLOOR, dtype=np.float64):
    """per problem, in long double from the inputs rounded to ``dtype``: the deviance D = 2 sum [y ln(y/ft) - (y - ft)] (the
    logarithmic term 0 for y <= 0), Pearson's X^2 = sum (y - ft)^2/ft with ft = max(f, floor), and the sums of absolute terms
    the error bounds of the device's fp64 accumulation are stated in: TD = sum (|y ln(y/ft)| + |y - ft| + |y|), TX = X^2"""
    T = np.dtype(dtype).type
    y = np.asarray(Y, dtype=dtype)
    f = np.asarray(F, dtype=dtype)
    ft = np.where(f < T(floor), T(floor), f).astype(L)
    y = y.astype(L)
    with np.errstate(all="ignore"):
        lg = np.where(y > 0, y * np.log(np.where(y > 0, y, 1) / ft), L(0))
        diff = y - ft
        D = 2 * (lg - diff).sum(-1)
        X = (diff * diff / ft).sum(-1)
        TD = (np.abs(lg) + np.abs(diff) + np.abs(y)).sum(-1)
    return D, X, TD, X


def sum_bound(m, vw):
    """|device sum - exact sum| <= sum_bound * eps64 * (sum of absolute terms).  A term: the quotient y/ft, the product with
    the logarithm, the difference and their sum are one rounding each (u = eps/2), the device logarithm is good to 1 ulp (2u
    of |ln|) and the rounding of the quotient moves ln by u, i.e. the product by u |y|: at most 4 u (|y ln| + |y - ft| + |y|);
    the X^2 term (difference, square, quotient) at most 3 u |term|.  The sum: a lane adds its ceil(m / (64 vw)) terms in
    order, six tree levels follow, each addition one rounding of a partial sum: (tiles + 6) u.  In units of eps = 2u and with
    the factor 2 of D: (4 + tiles + 6) u * 2 / 2u = 10 + tiles."""
    tiles = -(-m // (64 * vw))
    return 10 + tiles


# ---- workloads -----------------------------------------------------------------------------------------------------------
class Workload:
    """x, Y (counts), guess, truth, the device model and the two things the CPU side needs: ``oracle_fit(b, w, a0)`` ->
    (alpha, C, termination, n_evals, objective) and ``columns(alpha)`` -> (Phi (m, n), dPhi (m, q)) of one problem, dPhi[:, k]
    the derivative of basis function k by parameter k (both models: parameter k belongs to function k alone)"""


def double_exp(seed, B, m=200, peak=(30.0, 300.0)):
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, 20.0, m)
    truth = np.stack([rng.uniform(0.6, 1.2, B), rng.uniform(3.0, 5.0, B)], 1)
    A = np.exp(rng.uniform(np.log(peak[0]), np.log(peak[1]), B))
    c = np.stack([0.7 * A, 0.3 * A, rng.uniform(0.05, 0.3, B)], 1)
    Phi = np.stack([np.exp(-x[None] / truth[:, :1]), np.exp(-x[None] / truth[:, 1:]), np.ones((B, m))], 2)
    mean = np.einsum("bmn,bn->bm", Phi, c)
    wl = Workload()
    wl.name, wl.x, wl.mean, wl.truth, wl.c_true = "double_exp", x, mean, truth, c
    wl.Y = rng.poisson(mean).astype(np.float64)
    wl.guess = truth * (1 + rng.uniform(-0.1, 0.1, truth.shape))
    wl.n, wl.q, wl.irf = 3, 2, None
    wl.model = lambda dtype=np.float64: vp.multi_exponential_model(x, [1.0, 4.0], dtype=dtype)
    mdl = wl.model()

    def oracle_fit(b, w, a0):
        a, C, rep, _ = O.fit_batch(mdl, x, wl.Y[b:b + 1], a0[None], w=w)
        return a[0], C[0], int(rep["termination"][0]), int(rep["n_evals"][0]), float(rep["objective"][0])

    def columns(alpha):
        e1, e2 = np.exp(-x / alpha[0]), np.exp(-x / alpha[1])
        return (np.stack([e1, e2, np.ones(m)], 1), np.stack([e1 * x / alpha[0] ** 2, e2 * x / alpha[1] ** 2], 1))

    wl.oracle_fit, wl.columns = oracle_fit, columns
    return wl


def lifetime(seed, B, m=200, peak=(30.0, 300.0)):
    from test_gpu_external import oracle_problem
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, ic.WINDOW, m)
    dt = ic.grid_step(x)
    irf = ic.response(m, centre=0.08, width=0.012)
    truth = np.stack([rng.uniform(0.5, 1.5, B), rng.uniform(3.0, 6.0, B)], 1)
    c = rng.uniform(0.5, 2.0, (B, 4)) * np.array([10.0, 4.0, 3.0, 0.02])
    Phi = np.stack([ic.lifetime_columns(irf, dt, truth[b]) for b in range(B)])
    mean = np.einsum("bmn,bn->bm", Phi, c)
    A = np.exp(rng.uniform(np.log(peak[0]), np.log(peak[1]), B))
    scale = A / mean.max(1)
    mean, c = mean * scale[:, None], c * scale[:, None]
    wl = Workload()
    wl.name, wl.x, wl.mean, wl.truth, wl.c_true = "lifetime", x, mean, truth, c
    wl.Y = rng.poisson(mean).astype(np.float64)
    wl.guess = truth * (1 + rng.uniform(-0.1, 0.1, truth.shape))
    wl.n, wl.q, wl.irf = 4, 2, irf
    wl.model = lambda dtype=np.float64: ic.lifetime_model(x, dtype=dtype)
    cm = ic.lifetime_closures(x, irf)

    def oracle_fit(b, w, a0):
        p = oracle_problem(cm, wl.Y[b], w=w)
        p.set_params(a0)
        rep = p.fit()
        C = p.linear_coefficients()
        return p.params(), (C if C is not None else np.full(4, np.nan)), int(rep.termination), int(rep.n_evals), float(rep.objective)

    def columns(alpha):
        F1, _H1, D1 = ic.recurrence(irf, dt, alpha[0])
        F2, _H2, D2 = ic.recurrence(irf, dt, alpha[1])
        return np.stack([F1, F2, irf, np.ones(m)], 1), np.stack([D1, D2], 1)

    wl.oracle_fit, wl.columns = oracle_fit, columns
    return wl


def best_fit(wl, alpha, C):
    return np.stack([wl.columns(alpha[b])[0] @ C[b] for b in range(alpha.shape[0])])


def oracle_round(wl, W, a0):
    """one weighted fit of every problem on the oracle: (alpha (B, q), C (B, n), termination, n_evals, objective)"""
    B = wl.Y.shape[0]
    out = [wl.oracle_fit(b, None if W is None else W[b], np.asarray(a0[b], dtype=np.float64)) for b in range(B)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32),
            np.array([o[3] for o in out], dtype=np.int32), np.array([o[4] for o in out]))


def iterated_fit(wl, rounds, floor=FLOOR):
    """BatchProblem.fit_poisson on the CPU: a Neyman-weighted fit from the guess, then ``rounds`` fits with the mirror's
    weights of the previous fit, each from the previous parameters.  Returns the list of (alpha, C, termination) after
    every fit (rounds + 1 entries) -- the convergence sequence"""
    W, _ = reweight_mirror(wl.Y, None, floor)
    seq, a = [], wl.guess
    for r in range(rounds + 1):
        a, C, term, _nev, _obj = oracle_round(wl, W, a)
        seq.append((a, C, term))
        W, _ = reweight_mirror(wl.Y, best_fit(wl, a, C), floor)
    return seq


def relative_change(a_new, a_old):
    """per problem max_k |a_new - a_old| / max_k |a_new|: the measure of the existing parameter contract"""
    return (np.abs(a_new - a_old) / np.abs(a_new).max(1, keepdims=True)).max(1)


def normalised_score(wl, alpha, C, floor=FLOOR, Y=None):
    """per problem max_k |sum (y - f)/ft g_k| / sqrt(sum g_k^2/ft) over the columns g of [Phi, df/dalpha], ft = max(f, floor)
    (the variance the weights are formed from: the fixed point of the floored iteration is this score = 0; it is the Poisson
    score wherever f >= floor).  Each component is the score in units of its own standard deviation under the model."""
    Y = wl.Y if Y is None else Y
    out = np.empty(alpha.shape[0])
    for b in range(alpha.shape[0]):
        Phi, dPhi = wl.columns(np.asarray(alpha[b], dtype=np.float64))
        c = np.asarray(C[b], dtype=np.float64)
        f = Phi @ c
        ft = np.maximum(f, floor)
        G = np.concatenate([Phi, dPhi * c[:wl.q][None, :]], 1)
        num = np.abs(((Y[b] - f) / ft) @ G)
        den = np.sqrt((G * G / ft[:, None]).sum(0))
        out[b] = (num / den).max()
    return out


# the workloads of the tests (seeds chosen so that every oracle fit of every round succeeds: tests/test_poisson_host.py checks)
DOUBLE_EXP_SEED, LIFETIME_SEED, B_FIT = 11, 12, 48
