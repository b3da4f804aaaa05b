"""Cases and references of the per-kernel-set tests of vp_statistics / vp_best_fit (tests/test_stats_cases_host.py,
tests/test_gpu_stats_sets.py, tools/stats_sets_probe.py).

Every case NAMES the compiled kernel set it is meant to reach -- the record of vp_debug_kernel_set, (dtype, family, a, b, c,
R, W, uses_gen_ws) -- and the GPU tier asserts it before anything else, so a case written for "the 12-row set" fails, rather
than quietly testing another set, after a change of the registrations.  The CPU tier checks the table against the registry.

Two references, both evaluated at the handle's OWN inputs cast to fp64 (for an fp32 handle: the fp32-rounded grid, weights,
data and alpha):
  * the oracle (oracle/varpro_oracle.c: FitStatistics::try_calculate on the normal equations in long double), pinned to the
    reference's lmfit / MATLAB fixtures by tests/test_statistics.py;
  * numpy_statistics: a plain numpy restatement by another route (QR of H = W [Phi, sum_k dPhi_k c]), run in fp64 to
    cross-check the oracle and in fp32 to measure what fp32 arithmetic gives on that very case.
References are computed once per case (functools.lru_cache) and returned read-only."""
import collections
import functools
import zlib

import numpy as np

from oracle import oracle as O
from varpro_amd import basis
from varpro_amd._lib import FAMILY_GENERIC, FAMILY_MULTIEXP, FAMILY_RT
from varpro_amd.model import SeparableModel

EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
EPS_LONGDOUBLE = float(np.finfo(np.longdouble).eps)
F64, F32 = 0, 1  # VP_F64 / VP_F32
NP_DTYPE = {F64: np.float64, F32: np.float32}
BLK_R = 1 << 20  # rows per lane of the length-agnostic sets (vp_inst_blk.hpp)
B = 5
NOISE = 1e-3

# fp64 tolerances: the ones tests/test_statistics.py holds for the one set it covers
TOL64 = dict(chi2=1e-10, cov=1e-8, sigma=1e-8, best_fit=1e-10, cov_unit=1e-8, sigma_unit=1e-8)
# fp32: error <= FP32_MARGIN * max(e_np32, eps32 * kappa_s) (chi2: eps32 * sqrt(m)); e_np32 is the error of numpy_statistics
# run in fp32 on the case, kappa_s the condition number of the column-scaled H (first-order perturbation bound of a
# backward-stable QR).  The margin covers the device's different summation order.
# It is 64, not 8.  At 8, two cases missed on chi2, and through chi2 on Cov and sigma (generic fp32 single exponential m = 100
# weighted: largest ratio error / max(...) 25.0 on Cov, 20.4 on sigma, 16.0 on chi2; double exponential fp32 at dof = 1: 14.6
# on chi2; every other case <= 7.6; profiles/stats_sets_probe.json).  The cause is the order of the additions in one residual
# r_i = y_i - sum_j phi_ij c_j, which loses log10(|y_w| / |r_w|) ~ 3 digits to cancellation: chi2 = |r_w|^2 / dof of ONE
# problem is one draw of that rounding, not a bound of it.  Shown on the CPU, no device involved: with the SAME fp32 columns
# and the SAME c, taking the n multiply-adds of each row in another order moves numpy's own fp32 chi2 error of a problem of
# these two cases by up to 170x (3.4e-8 .. 5.9e-6, 3.8e-7 .. 1.4e-5, 3.1e-7 .. 1.4e-5); the device's largest, 1.9e-5 and
# 9.4e-5, sit at the upper end of those draws and a factor 5 and 2 under the first-order bound eps32 |y_w| / |r_w| (9.6e-5,
# 1.9e-4).  The kernels' own work does not share it: Cov / chi2 and sigma / sqrt(chi2) hold under FP32_UNIT_MARGIN = 8.
FP32_MARGIN = 64.0
FP32_UNIT_MARGIN = 8.0


# ---- kernel-set records ----------------------------------------------------------------------------------------------------
def me_set(dtype, nexp, offset, R, W=1):
    return (dtype, FAMILY_MULTIEXP, nexp, offset, 0, R, W, 0)


def rt_set(n, q, p, R, W=1):
    return (F64, FAMILY_RT, n, q, p, R, W, 0)


def blk_me_set(dtype, nexp, offset):
    return (dtype, FAMILY_MULTIEXP, nexp, offset, 0, BLK_R, 1, 1)


def blk_rt_set(n, q, p):
    return (F64, FAMILY_RT, n, q, p, BLK_R, 1, 1)


def gen_set(dtype):
    return (dtype, FAMILY_GENERIC, 0, 0, 0, 0, 1, 1)


def set_name(rec):
    dtype, fam, a, b, c, R, W, _gen = rec
    dt = "f64" if dtype == F64 else "f32"
    if fam == FAMILY_GENERIC:
        return "generic-%s" % dt
    shape = "me%d%s" % (a, "o" if b else "") if fam == FAMILY_MULTIEXP else "rt%d%d%d" % (a, b, c)
    return "%s-%s-%s" % (shape, dt, "blk" if R == BLK_R else "R%dW%d" % (R, W))


# ---- model shapes ----------------------------------------------------------------------------------------------------------
# kinds, parameter indices per basis function, the parameters the data are made with, grid span
Shape = collections.namedtuple("Shape", "kinds params truth span")
_E, _K, _C, _X, _S = basis.EXP_DECAY, basis.EXP_RATE, basis.CONST, basis.EXP_COS, basis.SIN_PHASE
# decay times: tests/test_gpu_streamed.py:_multiexp on 0 .. 12.5 for one to three exponentials; four on 0 .. 40; five a factor
# 3.2 apart on 0 .. 100 (kappa_s ~ 5e2; 0.3 .. 11 on 0 .. 40 gives 1.3e4, over the cap of tests/test_stats_cases_host.py)
_TAUS = {1: [2.0], 2: [1.0, 3.0], 3: [0.7, 2.0, 6.0], 4: [0.4, 1.6, 5.0, 14.0], 5: [0.3, 1.0, 3.2, 10.0, 32.0]}


def _me(nexp, offset):
    return Shape([_E] * nexp + ([_C] if offset else []), [(j,) for j in range(nexp)] + ([()] if offset else []),
                 _TAUS[nexp], {1: 12.5, 2: 12.5, 3: 12.5, 4: 40.0, 5: 100.0}[nexp])


SHAPES = {"me%d%s" % (k, "o" if off else ""): _me(k, off) for k in (1, 2, 3, 4, 5) for off in (0, 1)}
SHAPES.update({
    # run-time-descriptor shapes RtModel<N, Q, P>: the descriptors of tests/test_gpu_more.py, tests/models.py
    "rate1": Shape([_K], [(0,)], [0.8], 6.0),                                                  # (1, 1, 1)
    "rate1o": Shape([_K, _C], [(0,), ()], [0.9], 6.0),                                         # (2, 1, 1)
    "rate2": Shape([_K, _K], [(0,), (1,)], [0.4, 2.0], 6.0),                                   # (2, 2, 2)
    "cos1": Shape([_X], [(0, 1)], [0.4, 3.0], 6.0),                                            # (1, 2, 2)
    "dexp_unit": Shape([_E, _E, _C], [(1,), (0,), ()], [1.0, 3.0], 12.5),                      # (3, 2, 2) double_exp_unit_test_model
    "oleary": Shape([_X, _X], [(1, 2), (0, 1)], [1.0, 2.5, 4.0], 1.5),                         # (2, 3, 4) oleary_model: shared alpha2
    "cos2": Shape([_X, _X], [(0, 1), (2, 3)], [0.3, 2.0, 0.9, 5.0], 6.0),                      # (2, 4, 4)
    "rate3": Shape([_K] * 3, [(0,), (1,), (2,)], [0.3, 1.2, 4.0], 6.0),                        # (3, 3, 3)
    "rate3o": Shape([_K] * 3 + [_C], [(0,), (1,), (2,), ()], [0.3, 1.2, 4.0], 6.0),            # (4, 3, 3)
    "cos_rate2": Shape([_X, _K, _K], [(0, 1), (2,), (3,)], [0.4, 3.0, 0.2, 1.5], 6.0),         # (3, 4, 4)
    "cos_rate2o": Shape([_X, _K, _K, _C], [(0, 1), (2,), (3,), ()], [0.4, 3.0, 0.2, 1.5], 6.0),  # (4, 4, 4)
    # five exponentials a factor 4 apart on 0 .. 150: the fit case (at a factor 3.2 and noise 1e-3 one of the oracle's five
    # fits lets its longest decay time run off to 3e7, where H is singular to working precision)
    "me5o_wide": Shape([_E] * 5 + [_C], [(j,) for j in range(5)] + [()], [0.2, 0.8, 3.2, 12.8, 51.2], 150.0),
    # three exponentials a factor 4 apart on 0 .. 25: the fit cases of tests/fit_cases.py (at 0.7, 2, 6 on 0 .. 12.5 the minimum of
    # the oracle's own fit has kappa_s 1e4 .. 7e14 on five of the sizes there)
    "me3o_wide": Shape([_E] * 3 + [_C], [(0,), (1,), (2,), ()], [0.5, 2.0, 8.0], 25.0),
    # no set has this shape (q = 5): the generic kernels
    "mixed5": Shape([_E, _X, _S, _C], [(0,), (1, 2), (3, 4), ()], [1.5, 0.25, 2.0, 0.9, 0.4], 12.5),
})


def make_model(shape, x, dtype):
    s = SHAPES[shape]
    return SeparableModel(["a%d" % i for i in range(len(s.truth))], s.kinds, s.params, np.asarray(x, dtype=dtype), s.truth,
                          dtype=dtype)


# ---- the table -------------------------------------------------------------------------------------------------------------
# weights: None, "shared" (m,) or "per" (B, m); grid: "shared" (m,) or "per" (B, m); stream: stream_rows=True; uniform: the
# shared grid is np.linspace (True, every case of this file) or a jittered one the library's grid check rejects (False,
# tests/fit_cases.py; a per-problem grid is non-uniform whatever the flag says)
Case = collections.namedtuple("Case", "shape dtype m set weights grid stream noise uniform")


def case(shape, dtype, m, kset, weights=None, grid="shared", stream=False, noise=NOISE, uniform=True):
    return Case(shape, dtype, m, kset, weights, grid, stream, noise, uniform)


def case_id(c):
    return "%s-m%d-%s%s%s%s%s" % (c.shape, c.m, "f64" if c.dtype == F64 else "f32", {None: "", "shared": "-w", "per": "-wB"}[c.weights],
                                  "-tB" if c.grid == "per" else "", "-stream" if c.stream else "",
                                  "" if c.uniform else "-nu") + ("" if c.noise == NOISE else "-noise%g" % c.noise) + "@" + set_name(c.set)


def _seed(c):
    """the seed of a case's data: the record without the `uniform` field where that is the default, so that the cases older
    than the field keep their data bit for bit"""
    return zlib.crc32(repr(tuple(c)[:8] if c.uniform else tuple(c)).encode())


def _rt_cases(shape, n, q, p, sizes, blk_m):
    """one case per rows-per-lane R of a run-time shape (m that does not fill the set), one for its length-agnostic set"""
    m_of = {2: 100, 4: 200, 8: 400, 12: 700, 16: 900}
    out = [case(shape, F64, m_of[R], rt_set(n, q, p, R), weights="shared" if i % 2 else None) for i, R in enumerate(sizes)]
    return out + [case(shape, F64, blk_m, blk_rt_set(n, q, p))]


CASES = [
    # double exponential + offset, fp64: 2 / 2 (full) / 4 / 8 / 12 / 16 / 20 / 20 (full) rows per lane, then length-agnostic
    case("me2o", F64, 127, me_set(F64, 2, 1, 2)),
    case("me2o", F64, 128, me_set(F64, 2, 1, 2), weights="shared"),
    case("me2o", F64, 129, me_set(F64, 2, 1, 4)),
    case("me2o", F64, 300, me_set(F64, 2, 1, 8), weights="shared"),
    case("me2o", F64, 513, me_set(F64, 2, 1, 12)),
    case("me2o", F64, 769, me_set(F64, 2, 1, 16), weights="shared"),
    case("me2o", F64, 1025, me_set(F64, 2, 1, 20)),
    case("me2o", F64, 1280, me_set(F64, 2, 1, 20), weights="shared"),
    case("me2o", F64, 1281, blk_me_set(F64, 2, 1)),
    case("me2o", F64, 300, blk_me_set(F64, 2, 1), weights="shared", stream=True),
    # single exponential with / without offset
    case("me1o", F64, 100, me_set(F64, 1, 1, 2)),
    case("me1o", F64, 400, me_set(F64, 1, 1, 8), weights="shared"),
    case("me1o", F64, 900, me_set(F64, 1, 1, 16)),
    case("me1o", F64, 1100, me_set(F64, 1, 1, 24), weights="shared"),
    case("me1o", F64, 1537, me_set(F64, 1, 1, 32)),
    case("me1o", F64, 2049, blk_me_set(F64, 1, 1)),
    case("me1", F64, 100, me_set(F64, 1, 0, 2), weights="shared"),
    case("me1", F64, 900, me_set(F64, 1, 0, 16)),
    case("me1", F64, 1025, blk_me_set(F64, 1, 0)),
    # double exponential without offset
    case("me2", F64, 100, me_set(F64, 2, 0, 2)),
    case("me2", F64, 900, me_set(F64, 2, 0, 16), weights="shared"),
    case("me2", F64, 1025, blk_me_set(F64, 2, 0)),
    # triple exponential + offset: one-wave sets, then the four-wave set (unweighted and weighted)
    case("me3o", F64, 100, me_set(F64, 3, 1, 2)),
    case("me3o", F64, 400, me_set(F64, 3, 1, 8), weights="shared"),
    case("me3o", F64, 900, me_set(F64, 3, 1, 16)),
    case("me3o", F64, 1100, me_set(F64, 3, 1, 20), weights="shared"),
    case("me3o", F64, 1281, me_set(F64, 3, 1, 8, 4)),
    case("me3o", F64, 2048, me_set(F64, 3, 1, 8, 4), weights="shared"),
    case("me3o", F64, 2049, blk_me_set(F64, 3, 1)),
    # triple exponential without offset: its one resident set, and one row beyond it
    case("me3", F64, 100, me_set(F64, 3, 0, 2), weights="shared"),
    case("me3", F64, 129, rt_set(3, 3, 3, 16)),
    case("me3", F64, 1025, blk_me_set(F64, 3, 0)),
    # four and five exponentials, fp64: length-agnostic sets only
    case("me4o", F64, 300, blk_me_set(F64, 4, 1)),
    case("me4", F64, 300, blk_me_set(F64, 4, 0), weights="shared"),
    case("me4", F64, 100, rt_set(4, 4, 4, 2)),  # (no resident set of its own family: the run-time set, as "me3" at 129)
    case("me5o", F64, 300, blk_me_set(F64, 5, 1)),
    case("me5", F64, 300, blk_me_set(F64, 5, 0), weights="shared"),
    # fp32 double exponential + offset at 2 / 8 / 16 rows per lane, then length-agnostic
    case("me2o", F32, 100, me_set(F32, 2, 1, 2)),
    case("me2o", F32, 400, me_set(F32, 2, 1, 8), weights="shared"),
    case("me2o", F32, 900, me_set(F32, 2, 1, 16)),
    case("me2o", F32, 1025, blk_me_set(F32, 2, 1), weights="shared"),
    # fp32 five exponentials + offset: the 2-row set, the Gram handle's four-wave Householder statistics, length-agnostic
    case("me5o", F32, 100, me_set(F32, 5, 1, 2)),
    case("me5o", F32, 129, me_set(F32, 5, 1, 16, 4), weights="shared"),
    case("me5o", F32, 4096, me_set(F32, 5, 1, 16, 4)),
    case("me5o", F32, 4097, blk_me_set(F32, 5, 1)),
    # the generic kernels in both dtypes
    case("mixed5", F64, 300, gen_set(F64), weights="shared"),
    case("mixed5", F32, 300, gen_set(F32)),
    case("me1o", F32, 100, gen_set(F32), weights="shared"),  # (no fp32 set of this shape)
]
# every RtModel<N, Q, P> at each of its R
CASES += _rt_cases("rate1", 1, 1, 1, (2, 16), 1025)
CASES += _rt_cases("rate1o", 2, 1, 1, (2, 16), 1025)
CASES += _rt_cases("rate2", 2, 2, 2, (2, 16), 1025)
CASES += _rt_cases("cos1", 1, 2, 2, (2, 16), 1025)
CASES += _rt_cases("cos2", 2, 4, 4, (2, 16), 1025)
CASES += _rt_cases("rate3", 3, 3, 3, (2, 16), 1025)
CASES += _rt_cases("rate3o", 4, 3, 3, (2,), 129)
CASES += _rt_cases("cos_rate2", 3, 4, 4, (2,), 129)
CASES += _rt_cases("cos_rate2o", 4, 4, 4, (2,), 129)
CASES += _rt_cases("dexp_unit", 3, 2, 2, (2, 4, 8, 12, 16), 1025)
CASES += _rt_cases("oleary", 2, 3, 4, (2, 4, 8, 12, 16), 1025)


# ---- data ------------------------------------------------------------------------------------------------------------------
def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def case_data(c):
    """the handle's inputs, in the handle's dtype: x (m,) or (B, m), Y (B, m), w None / (m,) / (B, m), alpha (B, q) = the
    truth times 1.00 .. 1.04 per problem; every problem has its own coefficients and noise (seed: the case)"""
    s, T = SHAPES[c.shape], NP_DTYPE[c.dtype]
    rng = np.random.default_rng(_seed(c))
    n, q = len(s.kinds), len(s.truth)
    x = np.linspace(0.0, s.span, c.m)
    if not c.uniform and c.grid != "per":  # every interior point moved by up to 0.4 of the spacing: still increasing
        x[1:-1] += 0.8 * (rng.random(c.m - 2) - 0.5) * s.span / (c.m - 1)
    if c.grid == "per":  # every problem its own span, every grid non-uniform
        x = np.stack([np.sort(rng.random(c.m)) * s.span * (1.0 + 0.05 * b) for b in range(B)])
    x = np.ascontiguousarray(x, dtype=T)
    mdl = make_model(c.shape, x if x.ndim == 1 else x[0], T)
    coef = rng.uniform(5.0, 50.0, (B, n))
    Y = np.stack([coef[b] @ O.eval_phi(mdl, x if x.ndim == 1 else x[b], s.truth) for b in range(B)])
    Y = Y + c.noise * np.abs(Y).max(1, keepdims=True) * rng.standard_normal(Y.shape)
    alpha = np.asarray(s.truth) * rng.uniform(1.0, 1.04, (B, q))
    w = {None: None, "shared": rng.uniform(0.5, 1.5, c.m), "per": rng.uniform(0.5, 1.5, (B, c.m))}[c.weights]
    return _frozen(dict(model=mdl, x=x, Y=np.ascontiguousarray(Y, dtype=T), alpha=np.ascontiguousarray(alpha, dtype=T),
                        w=None if w is None else np.ascontiguousarray(w, dtype=T)))


def problem_inputs(d, b):
    """(x, y, w) of problem b as fp64 copies of the handle's inputs"""
    x = d["x"] if d["x"].ndim == 1 else d["x"][b]
    w = None if d["w"] is None else (d["w"] if d["w"].ndim == 1 else d["w"][b])
    return x.astype(np.float64), d["Y"][b].astype(np.float64), None if w is None else w.astype(np.float64)


# ---- references ------------------------------------------------------------------------------------------------------------
def jacobian_of_model_function(model, x, alpha, c):
    """J = [Phi, (dPhi/dalpha_k c)_k], (m, n + q), unweighted, fp64 (model_function_jacobian)"""
    q = int(model.n_params)
    Phi = O.eval_phi(model, x, alpha).T
    return np.concatenate([Phi, np.stack([O.eval_dphi(model, x, alpha, k).T @ c for k in range(q)], 1)], 1)


def numpy_statistics(model, x, y, w, alpha, dtype):
    """FitStatistics::try_calculate restated in numpy, all arithmetic in `dtype` (the columns are evaluated in fp64 and
    rounded): c = lstsq(W Phi, W y); H = W [Phi, sum_k dPhi_k c] = Q R; Cov = chi2 R^-1 R^-T; sigma_i = sqrt(chi2)
    |R^-T j_i| with the unweighted rows j_i.  -> dict(cov, reduced_chi2, conf_sigma, dof) or None (dof <= 0)"""
    T = np.dtype(dtype).type
    q = int(model.n_params)
    Phi = np.ascontiguousarray(O.eval_phi(model, x, alpha).T, dtype=T)
    m, n = Phi.shape
    dof = m - n - q
    if dof <= 0:
        return None
    wv = np.ones(m, dtype=T) if w is None else np.asarray(w, dtype=T)
    Pw, yw = Phi * wv[:, None], np.asarray(y, dtype=T) * wv
    c = np.linalg.lstsq(Pw, yw, rcond=None)[0]
    r = yw - Pw @ c
    chi2 = T(r @ r) / T(dof)
    D = [np.ascontiguousarray(O.eval_dphi(model, x, alpha, k).T, dtype=T) for k in range(q)]
    J = np.concatenate([Phi, np.stack([Dk @ c for Dk in D], 1)], 1)
    R = np.linalg.qr(J * wv[:, None], mode="r")
    Ri = np.linalg.solve(R, np.eye(n + q, dtype=T))
    out = dict(cov=chi2 * (Ri @ Ri.T), reduced_chi2=chi2, conf_sigma=np.sqrt(chi2) * np.linalg.norm(J @ Ri, axis=1), dof=dof)
    assert all(np.asarray(v).dtype == np.dtype(dtype) for k, v in out.items() if k != "dof")
    return out


def errors(st, ref, colnorm):
    """the metric: scaled covariance D Cov D (D = column norms of H: dimensionless, small entries count) max-abs over the
    reference's max-abs; conf_sigma row by row over max |sigma_ref|; reduced chi2 relative.  cov_unit / sigma_unit: the same
    for Cov / chi2 and sigma / sqrt(chi2), each side divided by its OWN chi2 -- what the statistics kernel computes itself,
    free of the cost the evaluation cached"""
    D = np.outer(colnorm, colnorm)
    cov, sig, chi2 = np.asarray(st["cov"], dtype=np.float64), np.asarray(st["conf_sigma"], dtype=np.float64), float(st["reduced_chi2"])
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())  # noqa: E731
    return dict(cov=rel(cov * D, ref["cov"] * D), sigma=rel(sig, ref["conf_sigma"]),
                chi2=abs(chi2 - ref["reduced_chi2"]) / ref["reduced_chi2"],
                cov_unit=rel(cov * D / chi2, ref["cov"] * D / ref["reduced_chi2"]),
                sigma_unit=rel(sig / np.sqrt(chi2), ref["conf_sigma"] / np.sqrt(ref["reduced_chi2"])))


def reference_at(model, x, y, w, alpha, dtype):
    """everything the tests need of ONE problem at alpha (fp64 inputs): the oracle's statistics, best fit and residuals
    (None where the oracle reports a failure), the conditioning of H, the errors of numpy_statistics in fp64 and -- for an
    fp32 handle -- in fp32, and the tolerances that follow"""
    p = O.Problem(model, x, y, w=w)
    p.set_params(alpha)
    st, bf, r, c = p.statistics(), p.best_fit(), p.residuals(), p.linear_coefficients()
    out = dict(stats=st, best_fit=bf, residuals=r, n=len(model.kinds), m=x.size)
    if st is None:
        return out
    H = jacobian_of_model_function(model, x, alpha, c) * (1.0 if w is None else w[:, None])
    colnorm = np.linalg.norm(H, axis=0)
    out.update(colnorm=colnorm, kappa_s=float(np.linalg.cond(H / colnorm)), cond_H=float(np.linalg.cond(H)),
               e_np64=errors(numpy_statistics(model, x, y, w, alpha, np.float64), st, colnorm))
    if dtype == F64:
        out["tol"] = dict(TOL64)
    else:
        e32 = errors(numpy_statistics(model, x, y, w, alpha, np.float32), st, colnorm)
        floor = EPS32 * out["kappa_s"]
        out.update(e_np32=e32, tol=dict(cov=FP32_MARGIN * max(e32["cov"], floor), sigma=FP32_MARGIN * max(e32["sigma"], floor),
                                        chi2=FP32_MARGIN * max(e32["chi2"], EPS32 * np.sqrt(x.size)),
                                        best_fit=8.0 * EPS32 * out["n"],
                                        cov_unit=FP32_UNIT_MARGIN * max(e32["cov_unit"], floor),
                                        sigma_unit=FP32_UNIT_MARGIN * max(e32["sigma_unit"], floor)))
    return out


@functools.lru_cache(maxsize=None)
def reference(c):
    """reference_at for the B problems of a case at the case's alpha"""
    d = case_data(c)
    return tuple(reference_at(d["model"], *problem_inputs(d, b), d["alpha"][b].astype(np.float64), c.dtype) for b in range(B))


def device_errors(st, bf, b, ref, y):
    """errors of problem b of a device result (statistics() dict, best_fit() array) against reference_at's record"""
    e = errors(dict(cov=st["cov"][b], conf_sigma=st["conf_sigma"][b], reduced_chi2=st["reduced_chi2"][b]), ref["stats"],
               ref["colnorm"])
    e["best_fit"] = float(np.abs(np.asarray(bf[b], dtype=np.float64) - ref["best_fit"]).max() / np.abs(y).max())
    return e


# ---- per-problem grids and weights (t_stride, w_stride): one fp64 one-wave set, one fp32 set, the four-wave set ---------------
PER_PROBLEM_CASES = [
    case("me2o", F64, 127, me_set(F64, 2, 1, 2), weights="per", grid="per"),
    case("me2o", F32, 400, me_set(F32, 2, 1, 8), weights="per", grid="per"),
    case("me3o", F64, 1281, me_set(F64, 3, 1, 8, 4), weights="per", grid="per"),
]

# ---- the edge of the degrees of freedom: m = n + q + dof for dof = 1, 0, -1, one and two exponentials at the 2-row sets ----
DOF_EDGE_SETS = [("me1o", F64, me_set(F64, 1, 1, 2)), ("me2o", F64, me_set(F64, 2, 1, 2)), ("me2o", F32, me_set(F32, 2, 1, 2)),
                 ("me1o", F32, gen_set(F32))]  # (no fp32 set of the single exponential: the generic kernel's edge)


def dof_edge_case(shape, dtype, kset, dof):
    return case(shape, dtype, len(SHAPES[shape].kinds) + len(SHAPES[shape].truth) + dof, kset)


DOF_EDGE_CASES = [dof_edge_case(*s, dof=1) for s in DOF_EDGE_SETS]


# ---- fits before the statistics --------------------------------------------------------------------------------------------
# one per family: multi-exponential fp64, the fp32 Gram handle, O'Leary weighted, streamed.  noise 1e-3, guesses within 5 %
FIT_CASES = [
    case("me2o", F64, 600, me_set(F64, 2, 1, 12)),
    case("me5o_wide", F32, 1000, me_set(F32, 5, 1, 16, 4)),
    case("oleary", F64, 230, rt_set(2, 3, 4, 4), weights="shared"),
    case("me3o", F64, 700, blk_me_set(F64, 3, 1), stream=True),
]


@functools.lru_cache(maxsize=None)
def fit_guess(c):
    d = case_data(c)
    rng = np.random.default_rng(_seed(c) + 1)
    g = np.asarray(SHAPES[c.shape].truth) * rng.uniform(0.95, 1.05, d["alpha"].shape)
    g = np.ascontiguousarray(g, dtype=d["alpha"].dtype)
    g.setflags(write=False)
    return g
