"""Data and the numpy checkers of the shifted IRF kinds (tests/test_irf_shift_host.py, tests/test_gpu_irf_shift.py).

Convention (include/varpro_hip.h, "Shifted IRF reconvolution"): delta in grid units, s = delta/dt bins, positive: later; the
response is zero outside the record; g_i = r(i - s) with r the Catmull-Rom cubic through the samples:
    o = floor(-s), f = -s - o;   g_i = sum_{a=-1..2} w_a(f) irf_{i+o+a};   g'_i = dg_i/ddelta = -(1/dt) sum_a w'_a(f) irf_{i+o+a}
``shifted_long_double`` evaluates this definition in np.longdouble from the inputs as the library sees them (already rounded to
the dtype) and returns the units of the error rule beside it; ``varpro_amd.model.irf_shifted`` is the library's numpy
mirror in the dtype of the response -- the reference of the device's error and the model of the oracle's closures."""
import functools

import numpy as np

import irf_cases as ic
import varpro_amd as vp
from varpro_amd import basis
from varpro_amd.model import _kind_columns, irf_columns, irf_shifted

L = np.longdouble
SHIFT, SCATTER, PSHIFT = basis.EXP_DECAY_IRF_SHIFT, basis.IRF_SHIFT, basis.EXP_DECAY_IRF_PERIODIC_SHIFT


def weights(f):
    """(w_-1..w_2, w'_-1..w'_2) of the definition, in the type of f"""
    f2, f3 = f * f, f * f * f
    w = [(-f3 + 2 * f2 - f) / 2, (3 * f3 - 5 * f2 + 2) / 2, (-3 * f3 + 4 * f2 + f) / 2, (f3 - f2) / 2]
    d = [(-3 * f2 + 4 * f - 1) / 2, (9 * f2 - 10 * f) / 2, (-9 * f2 + 8 * f + 1) / 2, (3 * f2 - 2 * f) / 2]
    return w, d


def shifted_long_double(irf, dt, delta):
    """(g, g', U, U') in long double: the definition, and the units sum_a |w_a| |tap| and sum_a |w'_a| |tap| / dt"""
    v = np.asarray(irf).astype(L)
    m = v.size
    dt, delta = L(dt), L(delta)
    ns = -(delta / dt)
    o = int(np.floor(ns))
    w, d = weights(ns - np.floor(ns))
    g, dg, U, dU = (np.zeros(m, L) for _ in range(4))
    idx = np.arange(m)
    for a in range(4):
        k = idx + o + a - 1
        tap = np.where((k >= 0) & (k < m), v[np.clip(k, 0, m - 1)], L(0))
        g += w[a] * tap
        dg += d[a] * tap
        U += np.abs(w[a]) * np.abs(tap)
        dU += np.abs(d[a]) * np.abs(tap)
    return g, -dg / dt, U, dU / dt


def shift_errors(g, dg, irf, dt, delta, eps, ref=None):
    """max errors of g and g' in units of eps (1 + |s|) U_i (U'_i for g'); rows whose unit is 0 must be exactly 0"""
    gl, dgl, U, dU = ref if ref is not None else shifted_long_double(irf, dt, delta)
    s = abs(L(delta) / L(dt))
    out = []
    for got, want, unit in ((g, gl, U), (dg, dgl, dU)):
        got = np.asarray(got)
        zero = unit == 0
        assert (got[zero] == 0).all()
        err = np.abs(got.astype(L) - want)[~zero] / (L(eps) * (1 + s) * unit[~zero])
        out.append(float(err.max()) if err.size else 0.0)
    return tuple(out)


def shifted_columns(kind, irf, dt, tau, delta, period=None):
    """(Phi, dPhi/dtau, dPhi/ddelta) of one shifted decay (kind 12 / 14) by the library's numpy mirror"""
    per = (period or 0.0) if kind == PSHIFT else None
    g, dg = irf_shifted(irf, dt, delta)
    f, dtau = irf_columns(g, dt, tau, per)
    return f, dtau, irf_columns(dg, dt, tau, per)[0]


# ---- the shifted lifetime models ------------------------------------------------------------------------------------------
# scatter-free: c1 (g * exp tau1) + c2 (g * exp tau2) + c3            (n = 3, q = 3, p = 4: tau1, delta | tau2, delta)
# full:         c1 (g * exp tau1) + c2 (g * exp tau2) + c3 g + c4     (n = 4, q = 3, p = 5: ... | delta)
NAMES = ["tau1", "tau2", "delta"]


def shifted_model(x, kind=SHIFT, scatter=False, dtype=np.float64):
    b = (vp.SeparableModelBuilder(NAMES, dtype=dtype)
         .function(["tau1", "delta"], kind).partial_deriv("tau1").partial_deriv("delta")
         .function(["tau2", "delta"], kind).partial_deriv("tau2").partial_deriv("delta"))
    if scatter:
        b = b.function(["delta"], SCATTER).partial_deriv("delta")
    return b.invariant_function(basis.CONST).independent_variable(x).initial_parameters([1.0, 4.0, 0.0]).build()


def shifted_closures(x, irf, kind=SHIFT, scatter=False, period=None):
    """the same model as numpy closures built on the library's mirror (one evaluation per (tau, delta) is shared)"""
    x = np.asarray(x, dtype=np.float64)
    irf = np.asarray(irf, dtype=np.float64)
    dt = ic.grid_step(x)
    decay = functools.lru_cache(maxsize=8)(lambda tau, delta: shifted_columns(kind, irf, dt, tau, delta, period))
    resp = functools.lru_cache(maxsize=4)(lambda delta: irf_shifted(irf, dt, delta))
    cm = vp.ClosureModel(NAMES, x)
    for name in ("tau1", "tau2"):
        cm = (cm.function([name, "delta"], lambda x, t, d: decay(float(t), float(d))[0])
              .partial_deriv(name, lambda x, t, d: decay(float(t), float(d))[1])
              .partial_deriv("delta", lambda x, t, d: decay(float(t), float(d))[2]))
    if scatter:
        cm = (cm.function(["delta"], lambda x, d: resp(float(d))[0]).partial_deriv("delta", lambda x, d: resp(float(d))[1]))
    return cm.invariant_function(lambda x: np.ones_like(x))


def unshifted_closures(x, responses, kind=basis.EXP_DECAY_IRF, period=None):
    """two decays of kind 9 / 11 + constant over a given response: the model a fixed delta reduces the scatter-free one to"""
    x = np.asarray(x, dtype=np.float64)
    g = np.asarray(responses, dtype=np.float64)
    dt = ic.grid_step(x)
    cached = functools.lru_cache(maxsize=8)(lambda tau: _kind_columns(kind, x, tau, None, g, period))
    return (vp.ClosureModel(["tau1", "tau2"], x)
            .function(["tau1"], lambda x, t: cached(float(t))[0]).partial_deriv("tau1", lambda x, t: cached(float(t))[1][0])
            .function(["tau2"], lambda x, t: cached(float(t))[0]).partial_deriv("tau2", lambda x, t: cached(float(t))[1][0])
            .invariant_function(lambda x: np.ones_like(x)))


def unshifted_model(x, kind=basis.EXP_DECAY_IRF):
    return (vp.SeparableModelBuilder(["tau1", "tau2"])
            .function(["tau1"], kind).partial_deriv("tau1").function(["tau2"], kind).partial_deriv("tau2")
            .invariant_function(basis.CONST).independent_variable(x).initial_parameters([1.0, 4.0]).build())


def model_columns(irf, dt, alpha, kind=SHIFT, scatter=False, period=None):
    """(m, n) basis matrix at one (tau1, tau2, delta), fp64"""
    cols = [shifted_columns(kind, irf, dt, alpha[0], alpha[2], period)[0], shifted_columns(kind, irf, dt, alpha[1], alpha[2], period)[0]]
    if scatter:
        cols.append(irf_shifted(irf, dt, alpha[2])[0])
    return np.stack(cols + [np.ones_like(irf)], 1)


def shifted_data(seed, B, m, kind=SHIFT, scatter=False, S=1, noise=1e-2, window=None, width=None):
    """B problems on x = linspace(0, window, m) after tests/irf_periodic_cases.py: tau1 in [0.5, 1.5], tau2 in [3, 6], guesses
    10 % off; the true delta within +-1.5 bins, its guess 0.  The response is at least about 6 bins wide (width 0.03 of 200
    samples; 0.012 of 1030 is 12 bins): with a response of 2.4 bins the ripple of the interpolation makes local minima in
    delta.  window: 25 for kind 12, 12.5 (incomplete decays) for kind 14"""
    rng = np.random.default_rng(seed)
    if window is None:
        window = 12.5 if kind == PSHIFT else 25.0
    if width is None:
        width = 0.03 if m < 600 else 0.012
    x = np.linspace(0.0, window, m)
    dt = ic.grid_step(x)
    irf = ic.response(m, 0.08, width)
    truth = np.stack([rng.uniform(0.5, 1.5, B), rng.uniform(3.0, 6.0, B), rng.uniform(-1.5, 1.5, B) * dt], 1)
    n = 4 if scatter else 3
    scale = np.array([10.0, 4.0, 3.0, 1.0]) if scatter else np.array([10.0, 4.0, 1.0])
    c = rng.uniform(0.5, 2.0, (B, n) if S == 1 else (B, S, n)) * scale
    Phi = np.stack([model_columns(irf, dt, truth[b], kind, scatter) for b in range(B)])  # (B, m, n)
    Y = np.einsum("bmn,bn->bm", Phi, c) if S == 1 else np.einsum("bmn,bsn->bsm", Phi, c)
    Y = Y + noise * np.abs(Y).max(-1, keepdims=True) * rng.standard_normal(Y.shape)
    guess = truth * (1 + rng.uniform(-0.1, 0.1, truth.shape))
    guess[:, 2] = 0.0
    return dict(x=x, irf=irf, truth=truth, Y=Y, guess=guess, dt=dt)


def model_costs(irf, dt, cand, Y, kind=SHIFT):
    """numpy costs (B, K) of every candidate (K, 3) of the scatter-free model for a shared response: lstsq, 1/2 ||r||^2"""
    cost = np.empty((Y.shape[0], cand.shape[0]))
    for k in range(cand.shape[0]):
        P = model_columns(irf, dt, cand[k], kind)
        r = Y.T - P @ np.linalg.lstsq(P, Y.T, rcond=None)[0]
        cost[:, k] = 0.5 * (r * r).sum(0)
    return cost, (Y * Y).sum(1)
