"""Data and the numpy checker of the start-point search tests (tests/test_search_host.py, tests/test_gpu_search.py).

The checker is numpy in fp64: for every candidate ``lstsq`` on W Phi and the cost 1/2 ||r||^2, summed over the right-hand
sides.  Costs are computed once per case (functools.lru_cache) and shared by the tests that need them."""
import functools

import numpy as np

import varpro_amd as vp
from varpro_amd import basis
from varpro_amd.model import _kind_columns

EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)

TAU1 = (0.5, 1.0, 1.5, 2.0, 3.0)
TAU2 = (4.0, 5.5, 7.0, 9.0, 12.0)


def base_candidates():
    """{0.5, 1, 1.5, 2, 3} x {4, 5.5, 7, 9, 12} plus the rank-deficient (2, 2): K = 26"""
    return np.vstack([vp.candidate_grid(TAU1, TAU2), [[2.0, 2.0]]])


@functools.lru_cache(maxsize=None)
def base_data(m, B=67):
    """double exponential plus constant on x = linspace(0, 12.5, m): tau1 in [0.6, 2.8], tau2 in [4.2, 11], c in [0.5, 2]^3,
    Gaussian noise 1e-2; shared weights 0.5 + U(0, 1)"""
    rng = np.random.default_rng(7 + m)
    x = np.linspace(0, 12.5, m)
    truth = np.stack([rng.uniform(0.6, 2.8, B), rng.uniform(4.2, 11, B)], 1)
    c = rng.uniform(0.5, 2, (B, 3))
    phi = lambda a: np.stack([np.exp(-x / a[0]), np.exp(-x / a[1]), np.ones_like(x)], 1)  # noqa: E731
    Y = np.stack([phi(truth[b]) @ c[b] for b in range(B)]) + 1e-2 * rng.standard_normal((B, m))
    w = 0.5 + rng.random(m)
    for a in (x, Y, w, truth):
        a.setflags(write=False)
    return dict(x=x, Y=Y, w=w, truth=truth)


def double_exp_model(x, dtype=np.float64):
    return vp.multi_exponential_model(np.asarray(x, dtype=dtype), [1.0, 6.0], dtype=dtype)


def columns(model, x, alpha):
    """(m, n) unweighted basis matrix of a descriptor model at one parameter vector, numpy fp64"""
    x = np.asarray(x, dtype=np.float64)
    cols = []
    with np.errstate(all="ignore"):
        for kind, par in zip(model.kinds, model.param_indices):
            p = [float(alpha[i]) for i in par] + [0.0, 0.0]
            cols.append(_kind_columns(kind, x, p[0], p[1])[0])
    return np.stack(cols, 1)


def numpy_costs(model, x, cand, Y, w=None):
    """cost (B, K) float64 of every candidate of every problem: lstsq on W Phi, 1/2 ||r||^2 summed over the right-hand sides;
    inf for a candidate whose Phi is not finite.  x (m,) or (B, m); cand (K, q) or (B, K, q); Y (B, m) or (B, S, m);
    w None, (m,) or (B, m).  Returns (cost, |y_w|^2 (B,))."""
    Y = np.asarray(Y, dtype=np.float64)
    Y3 = Y[:, None, :] if Y.ndim == 2 else Y
    B, _S, m = Y3.shape
    x = np.asarray(x, dtype=np.float64)
    cand = np.asarray(cand, dtype=np.float64)
    w = None if w is None else np.asarray(w, dtype=np.float64)
    W = np.ones((B, m)) if w is None else np.broadcast_to(w, (B, m))
    Yw = Y3 * W[:, None, :]
    K = cand.shape[-2]
    cost = np.full((B, K), np.inf)
    shared = x.ndim == 1 and cand.ndim == 2 and (w is None or w.ndim == 1)
    for k in range(K):
        if shared:
            P = columns(model, x, cand[k]) * W[0][:, None]
            if not np.isfinite(P).all():
                continue
            rhs = Yw.reshape(-1, m).T
            r = rhs - P @ np.linalg.lstsq(P, rhs, rcond=None)[0]
            cost[:, k] = 0.5 * (r * r).sum(0).reshape(B, -1).sum(1)
            continue
        for b in range(B):
            P = columns(model, x if x.ndim == 1 else x[b], cand[k] if cand.ndim == 2 else cand[b, k]) * W[b][:, None]
            if not np.isfinite(P).all():
                continue
            r = Yw[b].T - P @ np.linalg.lstsq(P, Yw[b].T, rcond=None)[0]
            cost[b, k] = 0.5 * (r * r).sum()
    return cost, (Yw * Yw).sum(axis=(1, 2))


@functools.lru_cache(maxsize=None)
def base_costs(m, weighted):
    d = base_data(m)
    cost, y2 = numpy_costs(double_exp_model(d["x"]), d["x"], base_candidates(), d["Y"], d["w"] if weighted else None)
    cost.setflags(write=False)
    y2.setflags(write=False)
    return cost, y2


def score_bound(n, m, y2, eps=EPS64):
    """the standard dot-product error bound on a score: 8 n m eps |y_w|^2"""
    return 8.0 * n * m * eps * y2


def check_fp64(index, cost_out, cost_np, y2, n, m, tol, cap=0.02, floor=False):
    """the fp64 criterion.  index must equal numpy's argmin wherever best and second-best numpy costs differ by more than
    the bound (at most `cap` of the problems may be excluded; cap=None: not checked); the numpy cost of the chosen
    candidate is <= the numpy minimum + bound on EVERY problem; cost_out agrees with numpy to `tol`, relative.  floor=True
    (the m < n case alone, where every cost is rounding noise around zero) adds eps |y_w|^2 to that limit: the rounding
    of the data's own energy, below which no cost is resolved."""
    index = np.asarray(index)
    B, K = cost_np.shape
    assert index.shape == (B,) and index.dtype == np.int32
    assert ((index >= 0) & (index < K)).all(), index
    bound = score_bound(n, m, y2)
    srt = np.sort(cost_np, 1)
    gap = srt[:, 1] - srt[:, 0] if K > 1 else np.full(B, np.inf)
    decided = gap > bound
    chosen = cost_np[np.arange(B), index]
    excess = chosen - srt[:, 0]
    print("search fp64: B=%d K=%d n=%d m=%d  excluded %d  min gap %.3e  max bound %.3e  max excess/bound %.3e"
          % (B, K, n, m, int((~decided).sum()), float(gap.min()), float(bound.max()), float((excess / bound).max())))
    if cap is not None:
        assert (~decided).mean() <= cap, "gap rule excludes %d of %d problems" % (int((~decided).sum()), B)
    assert np.array_equal(index[decided], cost_np.argmin(1)[decided])
    assert (excess <= bound).all(), float((excess / bound).max())
    if cost_out is not None:
        err = np.abs(np.asarray(cost_out) - chosen)
        lim = tol * chosen + (EPS64 * y2 if floor else 0.0)
        print("search fp64: max |cost_out - numpy| / limit %.3e" % float((err / lim).max()))
        assert (err <= lim).all(), float((err / lim).max())


def check_fp32(index, cost_np, y2):
    """the fp32 criterion: the numpy cost of the chosen candidate exceeds the numpy minimum by at most 8 eps32 |y_w|^2.
    Returns the worst ratio excess / (eps32 |y_w|^2)."""
    index = np.asarray(index)
    B, K = cost_np.shape
    assert ((index >= 0) & (index < K)).all(), index
    excess = cost_np[np.arange(B), index] - cost_np.min(1)
    ratio = float((excess / (EPS32 * y2)).max())
    print("search fp32: B=%d K=%d  worst excess / (eps32 |y_w|^2) = %.4f  (limit 8)" % (B, K, ratio))
    assert ratio <= 8.0, ratio
    return ratio


# ---- the device-column model of case 5: Gaussian + Lorentzian + linear + constant (n = 4, q = 4) ------------------------
PEAK_WIDTHS = (0.6, 0.8)
PEAK_MU1 = (2.4, 2.7, 3.0, 3.3, 3.6)
PEAK_MU2 = (5.9, 6.2, 6.5, 6.8, 7.1)


def peaks_model(x, dtype=np.float64):
    return (vp.SeparableModelBuilder(["mu1", "s1", "mu2", "g2"], dtype=dtype)
            .function(["mu1", "s1"], basis.GAUSS).partial_deriv("mu1").partial_deriv("s1")
            .function(["mu2", "g2"], basis.LORENTZ).partial_deriv("mu2").partial_deriv("g2")
            .invariant_function(basis.LINEAR).invariant_function(basis.CONST)
            .independent_variable(x).initial_parameters([3.0, 0.6, 6.5, 0.8]).build())


def peaks_candidates():
    """a grid over the two centres at fixed widths: K = 25"""
    return np.array([[a, PEAK_WIDTHS[0], b, PEAK_WIDTHS[1]] for a in PEAK_MU1 for b in PEAK_MU2])


@functools.lru_cache(maxsize=None)
def peaks_data(m=200, B=50):
    rng = np.random.default_rng(4100 + m)
    x = np.linspace(0.0, 10.0, m)
    mu1, s1 = rng.uniform(2.5, 3.5, B), rng.uniform(0.45, 0.8, B)
    mu2, g2 = rng.uniform(6.0, 7.0, B), rng.uniform(0.6, 1.1, B)
    c = np.stack([rng.uniform(5, 50, B), rng.uniform(5, 50, B), rng.uniform(-0.5, 0.5, B), rng.uniform(0, 5, B)], 1)
    mdl = peaks_model(x)
    Y = np.stack([columns(mdl, x, (mu1[b], s1[b], mu2[b], g2[b])) @ c[b] for b in range(B)])
    Y = Y + 1e-3 * np.abs(Y).max(1, keepdims=True) * rng.standard_normal(Y.shape)
    for a in (x, Y):
        a.setflags(write=False)
    return dict(x=x, Y=Y)


# ---- n = 8 on a generic-shape descriptor: three sine / cosine pairs, a decay and a constant (q = 6) ----------------------
def eight_basis_model(x):
    b = vp.SeparableModelBuilder(["w1", "w2", "w3", "pa", "pb", "tau"])
    for wn in ("w1", "w2", "w3"):
        for ph in ("pa", "pb"):
            b = b.function([wn, ph], basis.SIN_PHASE).partial_deriv(wn).partial_deriv(ph)
    b = b.function(["tau"], basis.EXP_DECAY).partial_deriv("tau").invariant_function(basis.CONST)
    return b.independent_variable(x).initial_parameters([1.0, 2.3, 3.9, 0.0, np.pi / 2, 3.0]).build()


def eight_basis_candidates():
    return np.array([[w1, 2.3, 3.9, 0.0, np.pi / 2, tau] for w1 in (0.8, 0.9, 1.0, 1.1, 1.2) for tau in (2.0, 3.0, 4.5)])


@functools.lru_cache(maxsize=None)
def eight_basis_data(m=75, B=21):
    rng = np.random.default_rng(88)
    x = np.linspace(0.0, 12.5, m)
    mdl = eight_basis_model(x)
    w1, tau = rng.uniform(0.82, 1.18, B), rng.uniform(2.1, 4.3, B)
    c = rng.uniform(0.5, 2.0, (B, 8))
    Y = np.stack([columns(mdl, x, (w1[b], 2.3, 3.9, 0.0, np.pi / 2, tau[b])) @ c[b] for b in range(B)])
    Y = Y + 1e-2 * rng.standard_normal(Y.shape)
    for a in (x, Y):
        a.setflags(write=False)
    return dict(x=x, Y=Y)
