"""Models, masks, numpy mirrors and data of the fixed-parameter tests (tests/test_fixed_host.py, tests/test_gpu_fixed.py).

A case is a descriptor model (full parameter order), the numpy closures of the same FULL model, and the names of the
parameters that are held.  ``Reduced`` is the mirror of what the device handle is: the closures of the reduced model over
the free parameters in model order, the fixed values embedded -- the model the CPU oracle fits.  The data and guesses of
the fit cases are those tests/test_gpu_bounds.py (peaks: rng 100 + m), tests/test_gpu_irf.py (lifetimes: seed 20 + m + S)
and tests/test_gpu_irf_periodic.py (seed 21 + m + S) hold their evaluation-count contracts on: 48 problems, m = 200,
separated lifetimes tau1 in [0.5, 1.5], tau2 in [3, 6], guesses 10 % off."""
import functools

import numpy as np

import irf_cases as ic
import irf_periodic_cases as pc
import varpro_amd as vp
from varpro_amd import basis
from test_gpu_external import gauss, gauss_dmu, gauss_dsg, lorentz, lorentz_dga, lorentz_dmu, peaks_data

B_FIT, M_FIT = 48, 200


class Reduced:
    """closures of the reduced model: ``cm`` (a ClosureModel of the full model) evaluated at the full vector made of the free
    parameters (model order) and the fixed ``values`` ((q,), full order; entries of free parameters are ignored); derivative
    columns of the free pairs only, numbered by counting free pairs"""

    def __init__(self, cm, names, fixed_names, values):
        self.cm, self.x = cm, cm.x
        self.names = list(names)
        self.held = np.array([self.names.index(k) for k in self.names if k in fixed_names], dtype=np.intp)
        self.free = np.array([k for k in range(len(self.names)) if k not in set(self.held.tolist())], dtype=np.intp)
        self.values = np.asarray(values, dtype=np.float64)
        assert self.values.shape == (len(self.names),)
        new_index = {int(k): i for i, k in enumerate(self.free)}
        self.keep = [p for p, (_j, k) in enumerate(cm.pairs()) if k in new_index]
        self._pairs = [(j, new_index[k]) for _j, (j, k) in enumerate(cm.pairs()) if k in new_index]

    def expand(self, a_free):
        a_free = np.asarray(a_free, dtype=np.float64).reshape(-1, self.free.size)
        full = np.tile(self.values, (a_free.shape[0], 1))
        full[:, self.free] = a_free
        return full

    def pairs(self):
        return list(self._pairs)

    def shape(self):
        return vp.ExternalModel(self.cm.shape().n_basis, int(self.free.size), self._pairs)

    def eval_batch(self, a_free):
        return self.cm.eval_batch(self.expand(a_free))

    def derivs_batch(self, a_free):
        return self.cm.derivs_batch(self.expand(a_free))[:, self.keep]


# ---- (a) the peaks model of the README: Gaussian + Lorentzian + linear + const, both widths fixed --------------------------
PEAK_NAMES = ["mu1", "s1", "mu2", "g2"]


def peaks_model(x, dtype=np.float64):
    return (vp.SeparableModelBuilder(PEAK_NAMES, dtype=dtype)
            .function(["mu1", "s1"], basis.GAUSS).partial_deriv("mu1").partial_deriv("s1")
            .function(["mu2", "g2"], basis.LORENTZ).partial_deriv("mu2").partial_deriv("g2")
            .invariant_function(basis.LINEAR).invariant_function(basis.CONST)
            .independent_variable(x).initial_parameters([3.0, 0.7, 6.4, 0.9]).build())


def peaks_closures(x):
    return (vp.ClosureModel(PEAK_NAMES, x)
            .function(["mu1", "s1"], gauss).partial_deriv("mu1", gauss_dmu).partial_deriv("s1", gauss_dsg)
            .function(["mu2", "g2"], lorentz).partial_deriv("mu2", lorentz_dmu).partial_deriv("g2", lorentz_dga)
            .invariant_function(lambda x: x.copy())
            .invariant_function(lambda x: np.ones_like(x)))


# ---- (d) a descriptor built to break pair counting ---------------------------------------------------------------------
# f0 Gauss(mu1, s): mu1 free, s fixed and SHARED with f2;  f1 Lorentz(mu2, g2): BOTH fixed, between two functions with free
# parameters;  f2 Gauss(mu3, s);  f3 the reconvolved decay with a free tau behind them;  f4 a pointwise decay behind the IRF
# function (a run of the column kernel whose dPhi starts at the free pairs in front of it);  f5 const
TRAP_NAMES = ["mu1", "s", "mu2", "g2", "mu3", "tau", "tau2"]
TRAP_FIXED = ("s", "mu2", "g2")


def trap_model(x, dtype=np.float64):
    return (vp.SeparableModelBuilder(TRAP_NAMES, dtype=dtype)
            .function(["mu1", "s"], basis.GAUSS).partial_deriv("mu1").partial_deriv("s")
            .function(["mu2", "g2"], basis.LORENTZ).partial_deriv("mu2").partial_deriv("g2")
            .function(["mu3", "s"], basis.GAUSS).partial_deriv("mu3").partial_deriv("s")
            .function(["tau"], basis.EXP_DECAY_IRF).partial_deriv("tau")
            .function(["tau2"], basis.EXP_DECAY).partial_deriv("tau2")
            .invariant_function(basis.CONST)
            .independent_variable(x).initial_parameters([2.0, 0.5, 5.0, 0.6, 8.0, 1.0, 3.0]).build())


def trap_closures(x, irf):
    x = np.asarray(x, dtype=np.float64)
    irf = np.asarray(irf, dtype=np.float64)
    dt = ic.grid_step(x)
    cached = functools.lru_cache(maxsize=8)(lambda tau: ic.recurrence(irf, dt, tau))
    return (vp.ClosureModel(TRAP_NAMES, x)
            .function(["mu1", "s"], gauss).partial_deriv("mu1", gauss_dmu).partial_deriv("s", gauss_dsg)
            .function(["mu2", "g2"], lorentz).partial_deriv("mu2", lorentz_dmu).partial_deriv("g2", lorentz_dga)
            .function(["mu3", "s"], gauss).partial_deriv("mu3", gauss_dmu).partial_deriv("s", gauss_dsg)
            .function(["tau"], lambda x, t: cached(float(t))[0]).partial_deriv("tau", lambda x, t: cached(float(t))[2])
            .function(["tau2"], lambda x, t: np.exp(-x / t)).partial_deriv("tau2", lambda x, t: np.exp(-x / t) * x / t ** 2)
            .invariant_function(lambda x: np.ones_like(x)))


def trap_data(seed, B, m, noise=1e-2):
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, 10.0, m)
    irf = ic.response(m, centre=0.08, width=0.012)
    truth = np.stack([rng.uniform(1.5, 2.5, B), rng.uniform(0.4, 0.7, B), rng.uniform(4.5, 5.5, B), rng.uniform(0.5, 0.8, B),
                      rng.uniform(7.5, 8.5, B), rng.uniform(0.4, 0.8, B), rng.uniform(2.0, 3.0, B)], 1)
    cm = trap_closures(x, irf)
    c = rng.uniform(0.5, 2.0, (B, 6)) * np.array([20.0, 20.0, 20.0, 5.0, 10.0, 1.0])
    Y = np.einsum("bn,bnm->bm", c, cm.eval_batch(truth)) if m > 1 else np.ones((B, m))
    Y = Y + noise * np.abs(Y).max(1, keepdims=True) * rng.standard_normal(Y.shape)
    guess = truth * (1 + rng.uniform(-0.1, 0.1, truth.shape))
    return dict(x=x, irf=irf, truth=truth, Y=Y, guess=guess, cm=cm)


# ---- (e) double exponential of the kinds 0..4 alone, tau1 fixed ---------------------------------------------------------
EXP_NAMES = ["tau1", "tau2"]


def double_exp_model(x, dtype=np.float64):
    return (vp.SeparableModelBuilder(EXP_NAMES, dtype=dtype)
            .function(["tau1"], basis.EXP_DECAY).partial_deriv("tau1")
            .function(["tau2"], basis.EXP_DECAY).partial_deriv("tau2")
            .invariant_function(basis.CONST)
            .independent_variable(x).initial_parameters([1.0, 4.0]).build())


def double_exp_closures(x):
    decay = lambda x, t: np.exp(-x / t)
    ddecay = lambda x, t: np.exp(-x / t) * x / t ** 2
    return (vp.ClosureModel(EXP_NAMES, x)
            .function(["tau1"], decay).partial_deriv("tau1", ddecay)
            .function(["tau2"], decay).partial_deriv("tau2", ddecay)
            .invariant_function(lambda x: np.ones_like(x)))


def double_exp_data(seed, B, m, noise=1e-2):
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, ic.WINDOW, m)
    truth = np.stack([rng.uniform(0.5, 1.5, B), rng.uniform(3.0, 6.0, B)], 1)
    c = rng.uniform(0.5, 2.0, (B, 3)) * np.array([10.0, 4.0, 1.0])
    Y = np.einsum("bn,bnm->bm", c, double_exp_closures(x).eval_batch(truth))
    Y = Y + noise * np.abs(Y).max(1, keepdims=True) * rng.standard_normal(Y.shape)
    guess = truth * (1 + rng.uniform(-0.1, 0.1, truth.shape))
    return dict(x=x, truth=truth, Y=Y, guess=guess)


# ---- the five cases ------------------------------------------------------------------------------------------------------
class Case:
    """one case on one grid: ``model(dtype)`` the descriptor, ``cm`` the full closures, ``names`` / ``fixed_names``, ``kwargs``
    of BatchProblem (irf, irf_period), and -- fit cases -- Y, guess (B, q) and truth"""

    def __init__(self, key, model, cm, names, fixed_names, kwargs=None, data=None):
        self.key, self.model, self.cm, self.names, self.fixed_names = key, model, cm, list(names), tuple(fixed_names)
        self.kwargs = kwargs or {}
        self.data = data
        self.held = [self.names.index(k) for k in self.names if k in self.fixed_names]
        self.free = [k for k in range(len(self.names)) if k not in self.held]
        self.free_pairs = [p for p, (_j, k) in enumerate(cm.pairs()) if k in self.free]

    def reduced(self, values):
        return Reduced(self.cm, self.names, self.fixed_names, values)

    def fixed_dict(self, values):
        """{name: value} for BatchProblem(fixed=...) from full-order values (q,) or (B, q)"""
        values = np.asarray(values)
        return {self.names[k]: (float(values[k]) if values.ndim == 1 else values[:, k].copy()) for k in self.held}


CASE_KEYS = ("a", "b", "c", "d", "e")
FIT_KEYS = ("a", "b", "c", "e")


def columns_case(key, m, B=5, seed=7):
    """a case for the column tests: any m >= 1, parameters (B, q) near the middle of their ranges.  The grids have a step of
    k/128: exactly representable in fp32, so that the rounded grid is uniform (the IRF kinds check it)"""
    rng = np.random.default_rng(seed + m)
    fine, coarse = np.arange(m) * (5.0 / 128.0), np.arange(m) * (12.0 / 128.0)
    if key == "a":
        x = fine
        alpha = np.array([3.0, 0.7, 6.4, 0.9]) * (1 + rng.uniform(-0.1, 0.1, (B, 4)))
        return Case(key, lambda dt=np.float64: peaks_model(x.astype(dt), dt), peaks_closures(x), PEAK_NAMES, ("s1", "g2")), x, alpha
    if key in ("b", "c"):
        x = coarse
        irf = ic.response(m, centre=0.08, width=0.012)
        alpha = np.array([1.0, 4.0]) * (1 + rng.uniform(-0.2, 0.2, (B, 2)))
        if key == "b":
            return Case(key, lambda dt=np.float64: ic.lifetime_model(x.astype(dt), dt), ic.lifetime_closures(x, irf),
                        EXP_NAMES, ("tau2",), dict(irf=irf)), x, alpha
        return Case(key, lambda dt=np.float64: pc.periodic_lifetime_model(x.astype(dt), dt),
                    pc.periodic_lifetime_closures(x, irf, None), EXP_NAMES, ("tau2",), dict(irf=irf)), x, alpha
    if key == "d":
        x = fine
        irf = ic.response(m, centre=0.08, width=0.012)
        alpha = np.array([2.0, 0.5, 5.0, 0.6, 8.0, 1.0, 3.0]) * (1 + rng.uniform(-0.1, 0.1, (B, 7)))
        return Case(key, lambda dt=np.float64: trap_model(x.astype(dt), dt), trap_closures(x, irf), TRAP_NAMES, TRAP_FIXED,
                    dict(irf=irf)), x, alpha
    x = coarse
    alpha = np.array([1.0, 4.0]) * (1 + rng.uniform(-0.2, 0.2, (B, 2)))
    return Case(key, lambda dt=np.float64: double_exp_model(x.astype(dt), dt), double_exp_closures(x), EXP_NAMES, ("tau1",)), x, alpha


@functools.lru_cache(maxsize=None)
def fit_case(key, weighted=False):
    """a fit case: 48 problems, m = 200; the fixed values are each problem's true values (per problem).  Returns
    (case, x, Y, guess (B, q), values (B, q), w); nothing in it is modified"""
    B, m = B_FIT, M_FIT
    if key == "a":
        rng = np.random.default_rng(100 + m)
        x = np.linspace(0.0, 10.0, m)
        truth, _c, Y, guess = peaks_data(rng, B, x, noise=1e-2)
        case = Case(key, lambda dt=np.float64: peaks_model(x.astype(dt), dt), peaks_closures(x), PEAK_NAMES, ("s1", "g2"))
    elif key == "b":
        d = ic.lifetime_data(20 + m + 1, B, m)
        x, truth, Y, guess = d["x"], d["truth"], d["Y"], d["guess"]
        case = Case(key, lambda dt=np.float64: ic.lifetime_model(x.astype(dt), dt), ic.lifetime_closures(x, d["irf"]), EXP_NAMES,
                    ("tau2",), dict(irf=d["irf"]))
    elif key == "c":
        d = pc.periodic_lifetime_data(21 + m + 1, B, m)
        x, truth, Y, guess = d["x"], d["truth"], d["Y"], d["guess"]
        case = Case(key, lambda dt=np.float64: pc.periodic_lifetime_model(x.astype(dt), dt),
                    pc.periodic_lifetime_closures(x, d["irf"], d["period"]), EXP_NAMES, ("tau2",),
                    dict(irf=d["irf"], irf_period=d["period"]))
    elif key == "e":
        d = double_exp_data(23, B, m)
        x, truth, Y, guess = d["x"], d["truth"], d["Y"], d["guess"]
        case = Case(key, lambda dt=np.float64: double_exp_model(x.astype(dt), dt), double_exp_closures(x), EXP_NAMES, ("tau1",))
    else:
        raise KeyError(key)
    w = (0.5 + np.random.default_rng(3 + m).random(m)) if weighted else None
    values = np.zeros_like(truth)
    values[:, case.held] = truth[:, case.held]
    for arr in (Y, guess, values) + ((w,) if weighted else ()):
        arr.setflags(write=False)
    return case, x, Y, guess, values, w


def reduced_oracle_fits(case, Y, guess, values, w=None):
    """(alpha_free (B, q_free), termination, n_evals, objective) of the oracle's fits of the reduced problems; values (q,) or
    (B, q)"""
    from test_gpu_extfit import oracle_fits
    values = np.asarray(values)
    g = np.asarray(guess)[:, case.free]
    if values.ndim == 1:
        return oracle_fits(case.reduced(values), Y, g, w)
    parts = [oracle_fits(case.reduced(values[b]), Y[b:b + 1], g[b:b + 1], w) for b in range(Y.shape[0])]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))


@functools.lru_cache(maxsize=None)
def fit_reference(key, weighted=False):
    """the reduced oracle's fits of ``fit_case(key, weighted)``: computed once, shared, never modified"""
    case, _x, Y, guess, values, w = fit_case(key, weighted)
    ref = reduced_oracle_fits(case, Y, guess, values, w)
    for arr in ref:
        arr.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def alternating_lifetime_case():
    """case (b) with fixed values that differ strongly between neighbouring problems: the true tau2 alternates between ~3 and
    ~6, so a value read by the slot of the compacted active list instead of the problem id belongs to another decay.
    Returns (case, x, Y, guess, values (B, q)); nothing in it is modified"""
    B, m = B_FIT, M_FIT
    d = ic.lifetime_data(20 + m + 1, B, m)
    rng = np.random.default_rng(5)
    truth = d["truth"].copy()
    truth[:, 1] = np.where(np.arange(B) % 2 == 0, 3.0, 6.0) * (1 + rng.uniform(-0.02, 0.02, B))
    c = rng.uniform(0.5, 2.0, (B, 4)) * np.array([10.0, 4.0, 3.0, 1.0])
    Phi = np.stack([ic.lifetime_columns(d["irf"], d["dt"], truth[b]) for b in range(B)])
    Y = np.einsum("bmn,bn->bm", Phi, c)
    Y = Y + 1e-2 * np.abs(Y).max(-1, keepdims=True) * rng.standard_normal(Y.shape)
    guess = truth * (1 + rng.uniform(-0.1, 0.1, truth.shape))
    x = d["x"]
    case = Case("b", lambda dt=np.float64: ic.lifetime_model(x.astype(dt), dt), ic.lifetime_closures(x, d["irf"]), EXP_NAMES,
                ("tau2",), dict(irf=d["irf"]))
    values = np.zeros_like(truth)
    values[:, 1] = truth[:, 1]
    for arr in (Y, guess, values):
        arr.setflags(write=False)
    return case, x, Y, guess, values
