"""GPU tier of the Poisson-weighted fits: the re-weighting kernel (varpro_amd/csrc/vp_poisson.hpp) against its numpy mirror,
vp_set_weights against a fresh handle, one re-weighted round and the whole iterated fit against the CPU oracle, and every
refusal.  Data, mirror and the CPU iterated fit: tests/poisson_cases.py; the CPU tier checks them in tests/test_poisson_host.py."""
import ctypes as C

import numpy as np
import pytest

import contracts as K
import poisson_cases as pc
import varpro_amd as vp
from varpro_amd import _lib
from varpro_amd.batch import POISSON_ROUNDS
from test_gpu_extfit import compare_with_oracle
from test_poisson_host import SCORE_BOUND

pytestmark = pytest.mark.gpu

L = np.longdouble


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


# ---- 1. the kernel against the mirror ------------------------------------------------------------------------------------
# How the kernel forms w = 1/sqrt(v): the compiler's full-precision square root -- within one unit in the last place,
# relative error <= eps -- then the correctly rounded division, eps/2.  The mirror (numpy, the same dtype) makes the same two
# operations correctly rounded, eps/2 each.  Both against the exact value: |w_dev - w_mirror| <= (1 + 1/2 + 1/2 + 1/2) eps |w|
# = 2.5 eps |w|, and with the one multiplication on either side |Yw_dev - Yw_mirror| <= 3.5 eps |Yw|.
W_UNITS, YW_UNITS = 2.5, 3.5


def _close(got, ref, units, eps):
    got, ref = _np(got), np.asarray(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    err = np.abs(got[ok].astype(L) - ref[ok].astype(L))
    assert (err <= units * L(eps) * np.abs(ref[ok].astype(L))).all(), float((err / (L(eps) * np.maximum(np.abs(ref[ok]), 1e-300))).max())


@pytest.mark.parametrize("device", ["host", "torch"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 130, 257, 1030])
@pytest.mark.parametrize("B", [1, 37])
def test_kernel_against_the_mirror(B, m, dtype, device):
    """a caller-evaluated handle with one column, so that the test chooses the best fit the weights are formed from: it
    runs negative and under the floor, the counts hold zeros; B = 37 adds a problem with a NaN count and a problem whose
    evaluation failed.  m = 63 .. 1030: element-wise and 16-byte paths (130 and 1030 are no multiple of the fp32 group), the
    tail of a tile, several tiles"""
    rng = np.random.default_rng(1000 * B + m)
    eps, vw, floor = np.finfo(dtype).eps, (2 if dtype == np.float64 else 4), 1.0
    shape = 6.0 * np.exp(-3.0 * np.arange(m) / max(m, 2)) - 0.8  # 5.2 .. -0.5
    Phi = (shape[None] * rng.uniform(0.5, 1.5, (B, 1)) + 0.05 * rng.standard_normal((B, m))).astype(dtype)
    Y = rng.poisson(np.maximum(3.0 * Phi, 0.0)).astype(dtype)
    if m == 1:
        Y = np.maximum(Y, 1)  # (a zero count would make the one-column fit zero)
    nan_b, bad_b = (5, 9) if B > 1 else (None, None)
    Phi_in = Phi.copy()
    if B > 1:
        Phi_in[bad_b, m // 2] = np.nan  # its evaluation is latched: status != 0
    Yn = Y.copy()
    if B > 1:
        Yn[nan_b, m // 3] = np.nan
    w0 = rng.uniform(0.5, 1.5, (B, m)).astype(dtype)
    if device == "torch":
        import torch
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")  # noqa: E731
    else:
        dev = lambda a: a  # noqa: E731
    alpha = np.ones((B, 1), dtype)
    Phi_d, dPhi_d = dev(Phi_in[:, None, :]), dev(np.zeros((B, 1, m), dtype))
    bp = vp.BatchProblem(vp.ExternalModel(1, 1, [(0, 0)], dtype=dtype), dev(Y), weights=dev(w0))
    assert np.array_equal(_np(bp.weighted_data()), w0 * Y)
    good = np.ones(B, bool)
    if B > 1:
        good[bad_b] = False

    # Neyman: from the counts alone; the NaN count goes through
    assert bp.poisson_reweight(dev(Yn), "neyman", floor) is None
    w_ref, yw_ref = pc.reweight_mirror(Yn, None, floor, dtype)
    assert (Yn == 0).any() or m == 1
    _close(bp.weighted_data(), yw_ref, YW_UNITS, eps)
    if B > 1:
        assert np.isnan(_np(bp.weighted_data())[nan_b, m // 3])

    # model: from the best fit of the evaluation at the Neyman weights of the clean counts
    bp.poisson_reweight(dev(Y), "neyman", floor)
    yw_before = _np(bp.weighted_data()).copy()
    bp.set_params_with_basis(dev(alpha), Phi_d, dPhi_d)
    st = _np(bp.status())
    assert ((st == 0) == good).all()
    F = _np(bp.best_fit())
    assert (F[good] < 0).any() or m < 63
    assert (F[good] < floor).any() or m == 1
    # (the Neyman weight of an empty bin does not show in Y_w = w * 0; it shows in the residual there, r = -w f, and must be
    # 1/sqrt(floor) = 1: an auxiliary check through one more product and the quotient, hence its own 8 eps)
    r = _np(bp.residuals())
    empty = (Y == 0) & good[:, None] & (np.abs(F) > 0.1)
    assert (np.abs(-r[empty] / F[empty] - 1.0) <= 8 * eps).all()
    D, X = bp.poisson_reweight(dev(Yn), "model", floor)
    D, X = _np(D), _np(X)
    w_ref, yw_ref = pc.reweight_mirror(Yn, F, floor, dtype)
    yw = _np(bp.weighted_data())
    _close(yw[good], yw_ref[good], YW_UNITS, eps)
    Dr, Xr, TD, TX = pc.goodness_mirror(Yn, F, floor, dtype)
    e64, k = np.finfo(np.float64).eps, pc.sum_bound(m, vw)
    finite = good.copy()
    if B > 1:
        finite[nan_b] = False
        assert np.isnan(D[nan_b]) and np.isnan(X[nan_b]) and np.isnan(yw[nan_b, m // 3])
        # the failed problem keeps its weights and weighted data, bit for bit, and gets NaN sums
        assert np.isnan(D[bad_b]) and np.isnan(X[bad_b]) and np.array_equal(yw[bad_b], yw_before[bad_b])
    errD = np.abs(D[finite].astype(L) - Dr[finite]) / (e64 * TD[finite])
    errX = np.abs(X[finite].astype(L) - Xr[finite]) / (e64 * np.maximum(TX[finite], L(1e-300)))
    assert errD.max() <= k and errX.max() <= k, (float(errD.max()), float(errX.max()), k)
    assert (D[finite] >= -k * e64 * np.asarray(TD[finite], np.float64)).all()
    # afterwards: the evaluation is gone, the parameters are not; the NaN count is latched at the next evaluation
    assert np.array_equal(_np(bp.params()), alpha)
    assert bp.residuals() is None
    bp.set_params_with_basis(dev(alpha), Phi_d, dPhi_d)
    st2 = _np(bp.status())
    if B > 1:
        assert st2[nan_b] != 0 and st2[bad_b] != 0
    assert (st2[finite] == 0).all()
    # the weights themselves: counts of one make Y_w = w exactly; they come from the best fit of THIS evaluation
    F2 = _np(bp.best_fit())
    ones = np.ones((B, m), dtype)
    bp.poisson_reweight(dev(ones), "model", floor)
    w_ref2, _ = pc.reweight_mirror(ones, F2, floor, dtype)
    w_dev = _np(bp.weighted_data())
    _close(w_dev[finite], w_ref2[finite], W_UNITS, eps)
    assert (w_dev[finite] <= 1.0 / np.sqrt(dtype(floor))).all() and (w_dev[finite] > 0).all()
    bp.close()


# ---- 2. vp_set_weights against a fresh handle ------------------------------------------------------------------------------
@pytest.mark.parametrize("device_columns", [False, True])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("per_problem", [False, True])
def test_set_weights_is_the_handle_created_with_those_weights(per_problem, S, device_columns):
    rng = np.random.default_rng(7 + S)
    B, m = 5, 130
    x = np.linspace(0.0, 10.0, m)
    mdl = vp.multi_exponential_model(x, [1.0, 4.0])
    alpha = np.stack([rng.uniform(0.6, 1.4, B), rng.uniform(3.0, 5.0, B)], 1)
    shape = (B, m) if S == 1 else (B, S, m)
    Y = rng.poisson(20.0 * np.exp(-x / 2.0) + 1.0, shape).astype(np.float64)
    w1, w2 = (rng.uniform(0.5, 1.5, (B, m) if per_problem else (m,)) for _ in range(2))
    bp = vp.BatchProblem(mdl, Y, weights=w1, device_columns=device_columns)
    first = bp.evaluate(alpha)
    bp.set_weights(w2, Y)
    assert bp.residuals() is None  # the cached evaluation is gone
    got = bp.evaluate(alpha)
    fresh = vp.BatchProblem(mdl, Y, weights=w2, device_columns=device_columns)
    ref = fresh.evaluate(alpha)
    for key in ("r", "J", "C", "cost", "status"):
        assert np.array_equal(got[key], ref[key]), key
    assert not np.array_equal(got["r"], first["r"])
    assert np.array_equal(bp.weighted_data(), fresh.weighted_data())
    bp.close()
    fresh.close()


# ---- 3. one re-weighted round against the oracle ---------------------------------------------------------------------------
def _workload(name):
    return pc.double_exp(pc.DOUBLE_EXP_SEED, pc.B_FIT) if name == "double_exp" else pc.lifetime(pc.LIFETIME_SEED, pc.B_FIT)


@pytest.mark.parametrize("name", ["double_exp", "lifetime"])
def test_one_round_against_the_oracle(name):
    """fit, poisson_reweight(model), fit: the second fit against the oracle's fit at the mirror's weights of the DEVICE's
    best fit, from the same start, under the contract of every other fit test (tests/contracts.py EXTFIT, unchanged)"""
    wl = _workload(name)
    bp = vp.BatchProblem(wl.model(), wl.Y, weights="neyman", irf=wl.irf)
    assert np.array_equal(bp.weighted_data(), pc.reweight_mirror(wl.Y, None)[1])
    a1, _C1, rep1 = bp.fit(wl.guess)
    assert (rep1["termination"] > 0).all()
    F = bp.best_fit()
    D, X = bp.poisson_reweight(wl.Y, "model")
    a2, C2, rep2 = bp.fit(a1)
    W, _ = pc.reweight_mirror(wl.Y, F)
    a_ref, _C_ref, term, nev, obj = pc.oracle_round(wl, W, a1)
    assert (term > 0).all()  # the oracle alone succeeds on every problem: none is excluded
    s = compare_with_oracle(rep2, a2, (a_ref, term, nev, obj))
    print("%s, one re-weighted round: %s" % (name, s))
    Dr, Xr, TD, TX = pc.goodness_mirror(wl.Y, F)
    k, e64 = pc.sum_bound(wl.Y.shape[1], 2), np.finfo(np.float64).eps
    assert (np.abs(D.astype(L) - Dr) <= k * e64 * TD).all() and (np.abs(X.astype(L) - Xr) <= k * e64 * TX).all()
    bp.close()


# ---- 4. fit_poisson end to end ---------------------------------------------------------------------------------------------
# What the device may add to the CPU bound on the normalised score.  A device fit may differ from the oracle's by what the
# existing contract allows: a relative objective difference of EXTFIT["objective_rel_max_max"] at worst and
# EXTFIT["objective_rel_median_max"] in the median.  Around the minimum of a round's weighted least-squares problem the
# objective rises by 1/2 d^T I d (I = J^T J, the Fisher information at these weights), the score of the displaced point is
# I d, and by Cauchy-Schwarz each component in units of its standard deviation is |e_k^T I d| / sqrt(I_kk) <= sqrt(d^T I d)
# = sqrt(2 rel objective).  The rounds contract such a displacement by the factor the CPU sequence shows, <= 1/5 per round,
# so what all earlier rounds leave is at most 1/(1 - 1/5) of one round's.  objective = the fit's reported 1/2 ||r_w||^2.
CONTRACTION = 0.2


def _score_allowance(objective, rel):
    return SCORE_BOUND + np.sqrt(2.0 * rel * objective) / (1.0 - CONTRACTION)


@pytest.mark.parametrize("name,device", [("double_exp", "host"), ("lifetime", "host"), ("lifetime", "torch")])
def test_fit_poisson_reaches_the_score_equations(name, device):
    wl = _workload(name)
    if device == "torch":
        import torch
        dev = lambda a: torch.as_tensor(a, device="cuda:0")  # noqa: E731
    else:
        dev = lambda a: a  # noqa: E731
    bp = vp.BatchProblem(wl.model(), dev(wl.Y), weights="neyman", irf=None if wl.irf is None else dev(wl.irf))
    a, Cc, rep, info = bp.fit_poisson(dev(wl.Y), dev(wl.guess))
    rep = vp.BatchProblem.report_to_numpy(rep)
    assert (rep["termination"] > 0).all() and info["rounds"] == POISSON_ROUNDS
    a, Cc, D = _np(a), _np(Cc), _np(info["deviance"])
    score = pc.normalised_score(wl, a, Cc)
    worst = _score_allowance(rep["objective"], K.EXTFIT["objective_rel_max_max"])
    typical = _score_allowance(np.median(rep["objective"]), K.EXTFIT["objective_rel_median_max"])
    print("%s/%s fit_poisson: normalised score max %.2e median %.2e (CPU bound %.0e, allowances %.2e / %.2e = margins %.0f / %.1f)"
          % (name, device, score.max(), np.median(score), SCORE_BOUND, worst.min(), typical, worst.min() / SCORE_BOUND, typical / SCORE_BOUND))
    assert (score <= worst).all() and np.median(score) <= typical
    # the handle's state is the returned parameters: statistics and best fit without a further call
    assert np.array_equal(_np(bp.params()), a)
    st = bp.statistics()
    assert (_np(st["status"]) == 0).all()
    assert np.abs(_np(bp.best_fit()) - pc.best_fit(wl, a, Cc)).max() <= 1e-6 * wl.Y.max()
    assert np.allclose(_np(info["reduced_deviance"]), D / (wl.Y.shape[1] - wl.n - wl.q), rtol=1e-15)
    # the deviance is the one of the returned point: the same chain by hand on a second handle (the kernels are
    # deterministic) stops before the last re-weight, and the mirror takes the device's best fit there
    b2 = vp.BatchProblem(wl.model(), wl.Y, weights="neyman", irf=wl.irf)
    b2.poisson_reweight(wl.Y, "neyman")
    a2, C2, _rep2 = b2.fit(wl.guess)
    for _ in range(POISSON_ROUNDS):
        b2.poisson_reweight(wl.Y, "model")
        a2, C2, _rep2 = b2.fit(a2)
    assert np.array_equal(a2, a) and np.array_equal(C2, Cc)
    F = b2.best_fit()
    D2, X2 = b2.poisson_reweight(wl.Y, "model")
    assert np.array_equal(D2, D) and np.array_equal(X2, _np(info["pearson"]))
    Dr, Xr, TD, TX = pc.goodness_mirror(wl.Y, F)
    k, e64 = pc.sum_bound(wl.Y.shape[1], 2), np.finfo(np.float64).eps
    assert (np.abs(D.astype(L) - Dr) <= k * e64 * TD).all() and (np.abs(X2.astype(L) - Xr) <= k * e64 * TX).all()
    b2.close()
    bp.close()


def test_fit_poisson_fp32():
    """fp32 handle, the double exponential.  The bound is derived like the fp64 one from the contract the project holds
    fp32 fits to (tests/contracts.py CFG4_ALL): at least same_success_class_min of the fits succeed, the relative objective
    difference is objective_rel_median_max in the median and within 1e-3 on share_objective_within_1e-3_min of them"""
    wl = _workload("double_exp")
    bp = vp.BatchProblem(wl.model(np.float32), wl.Y.astype(np.float32), weights="neyman")
    a, Cc, rep, info = bp.fit_poisson(wl.Y.astype(np.float32), wl.guess.astype(np.float32))
    ok = rep["termination"] > 0
    assert ok.mean() >= K.CFG4_ALL["same_success_class_min"]
    with np.errstate(all="ignore"):
        score = pc.normalised_score(wl, a.astype(np.float64), Cc.astype(np.float64))[ok]
    obj =np.median(rep["objective"][ok])
    typical = _score_allowance(obj, K.CFG4_ALL["objective_rel_median_max"])
    share = K.CFG4_ALL["share_objective_within_1e-3_min"]
    most = _score_allowance(obj, 1e-3)
    print("fp32 fit_poisson: %d of %d fits ok, normalised score median %.2e, %.0f %% quantile %.2e (allowances %.2e / %.2e)"
          % (ok.sum(), ok.size, np.median(score), 100 * share, np.quantile(score, share), typical, most))
    assert np.median(score) <= typical and np.quantile(score, share) <= most
    # ... which still tells the iterated fit from the Neyman fit it starts from
    b0 = vp.BatchProblem(wl.model(np.float32), wl.Y.astype(np.float32), weights="neyman")
    a0, C0, r0 = b0.fit(wl.guess.astype(np.float32))
    with np.errstate(all="ignore"):  # (a fit that failed has no coefficients: its score is not a number and is left out)
        neyman = pc.normalised_score(wl, a0.astype(np.float64), C0.astype(np.float64))[r0["termination"] > 0]
    assert np.median(neyman) > 5 * most
    D = info["deviance"][ok]
    assert np.isfinite(D).all() and (D > 0).all()
    b0.close()
    bp.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _refused(bp, code, call, evaluate):
    before = evaluate()
    assert call() == code, bp.lib.vp_last_error()
    after = evaluate()
    for key in ("r", "C", "cost", "status"):
        assert np.array_equal(before[key], after[key], equal_nan=(key != "status")), key


def test_refusals_leave_the_handle_as_it_was():
    rng = np.random.default_rng(3)
    B, m = 4, 65
    x = np.linspace(0.0, 10.0, m)
    mdl = vp.multi_exponential_model(x, [1.0, 4.0])
    alpha = np.tile([1.0, 4.0], (B, 1))
    Y = rng.poisson(20.0 * np.exp(-x / 2.0) + 1.0, (B, m)).astype(np.float64)
    w = rng.uniform(0.5, 1.5, (B, m))
    out = np.zeros(B)
    lib = vp.load_library()
    dbl = C.c_double
    INV, UNS = _lib.VP_ERR_INVALID, _lib.VP_ERR_UNSUPPORTED
    NEY, MOD = _lib.VP_POISSON_NEYMAN, _lib.VP_POISSON_MODEL

    bp = vp.BatchProblem(mdl, Y, weights=w)
    ev = lambda: bp.evaluate(alpha)  # noqa: E731
    h = bp._h
    _refused(bp, INV, lambda: lib.vp_set_weights(h, None, _ptr(Y)), ev)
    _refused(bp, INV, lambda: lib.vp_set_weights(h, _ptr(w), None), ev)
    _refused(bp, INV, lambda: lib.vp_poisson_reweight(h, None, NEY, dbl(1.0), None, None), ev)
    _refused(bp, INV, lambda: lib.vp_poisson_reweight(h, _ptr(Y), 2, dbl(1.0), None, None), ev)
    _refused(bp, INV, lambda: lib.vp_poisson_reweight(h, _ptr(Y), -1, dbl(1.0), None, None), ev)
    for floor in (0.0, -1.0, np.inf, np.nan):
        _refused(bp, INV, lambda: lib.vp_poisson_reweight(h, _ptr(Y), MOD, dbl(floor), None, None), ev)
    _refused(bp, INV, lambda: lib.vp_poisson_reweight(h, _ptr(Y), NEY, dbl(1.0), _ptr(out), None), ev)
    _refused(bp, INV, lambda: lib.vp_poisson_reweight(h, _ptr(Y), NEY, dbl(1.0), None, _ptr(out)), ev)
    bp.close()

    # model mode before any parameters are set: against the evaluation of a twin that was never asked
    bp, twin = vp.BatchProblem(mdl, Y, weights=w), vp.BatchProblem(mdl, Y, weights=w)
    assert lib.vp_poisson_reweight(bp._h, _ptr(Y), MOD, dbl(1.0), None, None) == INV
    e1, e2 = bp.evaluate(alpha), twin.evaluate(alpha)
    assert all(np.array_equal(e1[k], e2[k]) for k in ("r", "C", "cost", "status"))
    # ... and straight after a re-weighting (the evaluation is gone, although vp_params answers)
    bp.poisson_reweight(Y, "model")
    assert np.array_equal(bp.params(), alpha)
    assert lib.vp_poisson_reweight(bp._h, _ptr(Y), MOD, dbl(1.0), None, None) == INV
    bp.close()
    twin.close()

    # a handle without weights, and one with shared weights
    bp = vp.BatchProblem(mdl, Y)
    ev = lambda: bp.evaluate(alpha)  # noqa: E731
    _refused(bp, INV, lambda: lib.vp_set_weights(bp._h, _ptr(w), _ptr(Y)), ev)
    _refused(bp, INV, lambda: lib.vp_poisson_reweight(bp._h, _ptr(Y), NEY, dbl(1.0), None, None), ev)
    bp.close()
    bp = vp.BatchProblem(mdl, Y, weights=w[0])
    _refused(bp, INV, lambda: lib.vp_poisson_reweight(bp._h, _ptr(Y), NEY, dbl(1.0), None, None), lambda: bp.evaluate(alpha))
    bp.close()

    # S > 1: weights per right-hand side do not exist
    Y3 = np.stack([Y, Y + 1, Y + 2], 1)
    bp = vp.BatchProblem(mdl, Y3, weights=w)
    _refused(bp, UNS, lambda: lib.vp_poisson_reweight(bp._h, _ptr(Y3), NEY, dbl(1.0), None, None), lambda: bp.evaluate(alpha))
    bp.close()

    # m < n: the handle is padded
    x2 = x[:2].copy()
    bp = vp.BatchProblem(vp.multi_exponential_model(x2, [1.0, 4.0]), Y[:, :2].copy(), weights=w[:, :2].copy())
    ev = lambda: bp.evaluate(alpha)  # noqa: E731
    Ys, ws = Y[:, :2].copy(), w[:, :2].copy()
    _refused(bp, UNS, lambda: lib.vp_set_weights(bp._h, _ptr(ws), _ptr(Ys)), ev)
    _refused(bp, UNS, lambda: lib.vp_poisson_reweight(bp._h, _ptr(Ys), NEY, dbl(1.0), None, None), ev)
    bp.close()

    # a caller-evaluated handle: a stepped fit in progress, and model mode without columns at the current parameters
    def columns(a):
        a = np.asarray(a)
        Phi = np.stack([np.exp(-x[None] / a[:, :1]), np.exp(-x[None] / a[:, 1:]), np.ones((B, m))], 1)
        return Phi, np.stack([Phi[:, 0] * x / a[:, :1] ** 2, Phi[:, 1] * x / a[:, 1:] ** 2], 1)

    ext = vp.BatchProblem(vp.ExternalModel(3, 2, [(0, 0), (1, 1)]), Y, weights=w)
    twin = vp.BatchProblem(vp.ExternalModel(3, 2, [(0, 0), (1, 1)]), Y, weights=w)
    ext.fit_begin(alpha)
    assert lib.vp_set_weights(ext._h, _ptr(w), _ptr(Y)) == INV
    assert lib.vp_poisson_reweight(ext._h, _ptr(Y), NEY, dbl(1.0), None, None) == INV
    trial = alpha
    for _ in range(300):
        trial, _want, nact = ext.fit_step_with_basis(*columns(trial))
        if nact == 0:
            break
    a_fit, _Cf, _rf = ext.fit_end()
    assert lib.vp_poisson_reweight(ext._h, _ptr(Y), MOD, dbl(1.0), None, None) == INV  # (the fitted point's columns are not known)
    Phi, dPhi = columns(a_fit)
    e1, e2 = ext.evaluate_with_basis(a_fit, Phi, dPhi), twin.evaluate_with_basis(a_fit, Phi, dPhi)
    assert all(np.array_equal(e1[k], e2[k]) for k in ("r", "C", "cost", "status"))
    # ... with them, model mode works on a caller-evaluated handle (the best fit formed here on the host: to its rounding)
    D, X = ext.poisson_reweight(Y, "model")
    Dr, Xr, _TD, _TX = pc.goodness_mirror(Y, np.einsum("bnm,bn->bm", Phi, e1["C"]))
    assert np.allclose(D, np.asarray(Dr, np.float64), rtol=1e-9) and np.allclose(X, np.asarray(Xr, np.float64), rtol=1e-9)
    ext.close()
    twin.close()
