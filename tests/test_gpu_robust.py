"""GPU tier of the robust fits: the re-weighting kernel (varpro_amd/csrc/vp_robust.hpp) against its numpy mirror, its
independence of the launch geometry, vp_weights, one re-weighted round and the whole iterated fit against the CPU oracle, and
every refusal.  Data, mirror and the CPU iterated fit: tests/robust_cases.py; the CPU tier checks them in
tests/test_robust_host.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import contracts as K
import poisson_cases as pc
import robust_cases as rc
import varpro_amd as vp
from varpro_amd import _lib
from varpro_amd.batch import ROBUST_ROUNDS
from test_gpu_extfit import compare_with_oracle
from test_robust_host import CONTRACTION, ROBUST_SCORE_BOUND

pytestmark = pytest.mark.gpu

L = np.longdouble
LOSSES = ("huber", "cauchy", "tukey")
# the one length threshold of the selection (vp_robust.hpp RES_ROWS): up to 1024 rows the keys stay in registers, beyond
# they live in the problem's row of w.  1024 and 1025 are its two sides; 1030 and 5000 stream several tiles, 5000 as
# 16-byte groups in both dtypes, 1025 and 1030 (fp32) element-wise.
LENGTHS = [1, 2, 3, 63, 64, 65, 130, 257, 1024, 1025, 1030, 5000]


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _dev(device):
    if device == "torch":
        import torch
        return lambda a: torch.tensor(np.array(a), device="cuda:0")  # (a copy: the shared inputs are read-only)
    return lambda a: a


# ---- 1. the kernel against the mirror ------------------------------------------------------------------------------------
# e = w0 (y - f), the sort, the half-sum of the two middle elements and the product with 1.4826 are single correctly rounded
# operations with nothing to contract: the scale is the mirror's bit for bit.  So are u = |e|/s and t = u/k (the compiler's
# divisions are correctly rounded in both dtypes): the device and the mirror start the weight from the SAME u and t, and the
# bounds count, in the manner of W_UNITS of tests/test_gpu_poisson.py, the roundings after them on both sides against the
# exact function of that u -- device square root 1 eps (within one unit in the last place), every other operation eps/2:
#   Huber   k/u is the same number on both sides.  Device: sqrt 1, product with w0 1/2.  Mirror: 1/2, 1/2.          2.5
#   Cauchy  x = 1 + t t: 1/2 fused, 1 as product and sum (t^2 <= x).  1/x: 1/2 more, at most 1.5; the square root halves
#           it.  Device (either form): 0.75 + 1 + 1/2 = 2.25.  Mirror (product and sum): 0.75 + 1/2 + 1/2 = 1.75.    4
#   Tukey   1 - t, 1 + t, their product and the product with w0 are correctly rounded on both sides and no sum follows
#           a product: the weights are the mirror's bit for bit.                                                      0
# and Y_w = w y adds eps/2 on either side: one unit more.  Tukey's weight goes to 0 at t -> 1, the others stay within
# [sqrt(k/u), 1] of w0: the bound is relative to |w| (and |Y_w|), which for a bound of 0 is the same as relative to w0.
W_UNITS = {"huber": 2.5, "cauchy": 4.0, "tukey": 0.0}
YW_UNITS = {loss: units + 1.0 for loss, units in W_UNITS.items()}
NAN_B, BAD_B = 5, 9      # a NaN observation; an evaluation that fails
SIX_B, EQUAL_B, ZEROS_B, NEGZERO_B, EVEN_B, ODD_B = 3, 4, 6, 7, 1, 2


def _close(got, ref, units, eps, what):
    got, ref = _np(got), np.asarray(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    err = np.abs(got[ok].astype(L) - ref[ok].astype(L))
    worst = float((err / (L(eps) * np.maximum(np.abs(ref[ok]).astype(L), L(1e-300)))).max()) if ok.any() else 0.0
    print("%s: %.2f eps (bound %.1f)" % (what, worst, units))
    assert (err <= units * L(eps) * np.abs(ref[ok].astype(L))).all(), (what, worst)


@functools.lru_cache(maxsize=None)
def _inputs(B, m, dtype):
    """Phi (the one column), Y, Yn (with the NaN), the base weights and the handle's first weights.  Problems 3, 4, 6, 7 of
    B = 37 have a column that is 0 below row 0, so that f = 0 and e = w0 y there: the test writes their residuals."""
    dtype = np.dtype(dtype).type
    rng = np.random.default_rng(1000 * B + m)
    shape = 6.0 * np.exp(-3.0 * np.arange(m) / max(m, 2)) + 0.5
    Phi = (shape[None] * rng.uniform(0.5, 1.5, (B, 1))).astype(dtype)
    Y = (3.0 * Phi + rng.standard_normal((B, m)) * np.where(rng.random((B, m)) < 0.1, 8.0, 1.0)).astype(dtype)
    w0 = rng.uniform(0.5, 1.5, (B, m)).astype(dtype)
    if B > 1:
        rest = m - 1
        for b in (SIX_B, EQUAL_B, ZEROS_B, NEGZERO_B):
            Phi[b, 0], Phi[b, 1:], w0[b], Y[b, 0] = 1.0, 0.0, 1.0, 5.0
        # at most six distinct |e|, the two middle elements different: 2 below, 3 above, me even
        w0[SIX_B, 0] = 0.0
        me = rest - rest % 2
        w0[SIX_B, 1 + me:] = 0.0
        low, high = np.full(me // 2, 2.0), np.full(me // 2, 3.0)
        low[::3], low[1::5], high[::4], high[2::7] = 1.0, 0.5, 8.0, 13.0
        Y[SIX_B, 1:1 + me] = rng.permutation(np.concatenate([low, high]) * rng.choice([-1.0, 1.0], me))
        # all e equal (row 0 does not count)
        w0[EQUAL_B, 0], Y[EQUAL_B, 1:] = 0.0, -2.5
        # more than half of the e exactly 0: the scale is 0
        Y[ZEROS_B, 1:][rng.permutation(rest)[:rest // 2 + 2]] = 0.0
        # e = -0.0 entries among ordinary ones
        Y[NEGZERO_B, 1:][rng.permutation(rest)[:rest // 4]] = -0.0
        # rows of weight 0: the count of the others even in one problem, odd in the other
        for b, parity in ((EVEN_B, 0), (ODD_B, 1)):
            zero = rng.permutation(m)[:m // 5]
            if (m - zero.size) % 2 != parity and m > 1:
                zero = np.append(zero, np.setdiff1d(np.arange(m), zero)[0])
            w0[b, zero] = 0.0
    Phi_in, Yn = Phi.copy(), Y.copy()
    if B > 1:
        Phi_in[BAD_B, m // 2] = np.nan  # its evaluation is latched: status != 0
        Yn[NAN_B, m // 3] = np.nan
    w_first = rng.uniform(0.5, 1.5, (B, m)).astype(dtype)
    for a in (Phi_in, Y, Yn, w0, w_first):
        a.setflags(write=False)
    return Phi_in, Y, Yn, w0, w_first


def _evaluated(bp, dev, Phi_in, Y, w_first, dtype):
    """the handle at its first weights, evaluated: (status == 0, the best fit the next re-weighting is formed from)"""
    B, m = Y.shape
    bp.set_weights(dev(w_first), dev(Y))
    bp.set_params_with_basis(dev(np.ones((B, 1), dtype)), dev(Phi_in[:, None, :]), dev(np.zeros((B, 1, m), dtype)))
    return _np(bp.status()) == 0, _np(bp.best_fit())


def _check_against_mirror(bp, out, Yn, F, w0, loss, scale, good, dtype, what):
    B, m = Yn.shape
    eps, vw = np.finfo(dtype).eps, (2 if dtype == np.float64 else 4)
    s, rho = _np(out[0]), _np(out[1])
    w, yw = _np(bp.weights()), _np(bp.weighted_data())
    w_ref, yw_ref, s_ref, u_ref = rc.reweight_mirror(Yn, F, w0, loss, rc.K95[loss], scale, dtype)
    assert s.dtype == np.float64 and np.array_equal(s[good], s_ref[good].astype(np.float64), equal_nan=True), what
    _close(w[good], w_ref[good], W_UNITS[loss], eps, what + " w")
    _close(yw[good], yw_ref[good], YW_UNITS[loss], eps, what + " Yw")
    assert (np.abs(w[good]) <= np.abs(w0[good]))[~np.isnan(w_ref[good])].all()  # (omega <= 1)
    r_ref, mag = rc.rho_mirror(u_ref, loss, rc.K95[loss], dtype)
    fin = good & ~np.isnan(np.asarray(r_ref, np.float64))
    assert np.isnan(rho[good & ~fin]).all()
    err = np.abs(rho[fin].astype(L) - r_ref[fin]) / (np.finfo(np.float64).eps * np.maximum(mag[fin], L(1e-300)))
    print("%s rho: %.2f eps64 of the absolute terms (bound %.1f)" % (what, float(err.max()) if fin.any() else 0.0, rc.rho_bound(m, vw)))
    assert (err <= rc.rho_bound(m, vw)).all()
    return s_ref, w_ref


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("device", ["host", "torch"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("m", LENGTHS)
@pytest.mark.parametrize("B", [1, 37])
def test_kernel_against_the_mirror(B, m, dtype, device, loss):
    """a caller-evaluated handle with one column, so that the test chooses the best fit the residuals are taken from.
    B = 37 holds the special problems of _inputs, a problem with a NaN observation and one whose evaluation failed"""
    Phi_in, Y, Yn, w0, w_first = _inputs(B, m, dtype)
    dev = _dev(device)
    bp = vp.BatchProblem(vp.ExternalModel(1, 1, [(0, 0)], dtype=dtype), dev(Y), weights=dev(w_first))
    alpha = np.ones((B, 1), dtype)
    expect = np.ones(B, bool)
    if B > 1:
        expect[BAD_B] = False

    # the scale estimated per problem
    good, F = _evaluated(bp, dev, Phi_in, Y, w_first, dtype)
    assert np.array_equal(good, expect)
    w_before, yw_before = _np(bp.weights()).copy(), _np(bp.weighted_data()).copy()
    assert np.array_equal(w_before, w_first)
    out = bp.robust_reweight(dev(Yn), loss, base_weights=dev(w0))
    s_ref, w_ref = _check_against_mirror(bp, out, Yn, F, w0, loss, 0.0, good, dtype, "estimated scale")
    if B > 1:
        s, rho, w, yw = _np(out[0]), _np(out[1]), _np(bp.weights()), _np(bp.weighted_data())
        # the failed problem keeps its weights and weighted data, bit for bit, and gets NaN outputs
        assert np.isnan(s[BAD_B]) and np.isnan(rho[BAD_B])
        assert np.array_equal(w[BAD_B], w_before[BAD_B]) and np.array_equal(yw[BAD_B], yw_before[BAD_B])
        assert np.isnan(s[NAN_B]) and np.isnan(rho[NAN_B]) and np.isnan(w[NAN_B]).all()
        # what the special problems are there for
        if m >= 63:
            e = w0 * (Y - F)
            six = np.sort(np.abs(e[SIX_B][w0[SIX_B] != 0]))
            assert np.unique(six).size <= 6 and six.size % 2 == 0 and six[six.size // 2 - 1] != six[six.size // 2]
            assert np.unique(e[EQUAL_B][w0[EQUAL_B] != 0]).size == 1 and s[EQUAL_B] == dtype(rc.MAD_TO_SIGMA) * dtype(2.5)
            assert s[ZEROS_B] == 0 and rho[ZEROS_B] == 0 and np.array_equal(w[ZEROS_B], w0[ZEROS_B])
            assert np.array_equal(yw[ZEROS_B], w0[ZEROS_B] * Y[ZEROS_B])
            assert np.signbit(e[NEGZERO_B][e[NEGZERO_B] == 0]).any()
            assert s[NEGZERO_B] > 0
            assert (w0[EVEN_B] != 0).sum() % 2 == 0 and (w0[ODD_B] != 0).sum() % 2 == 1 and (w0[EVEN_B] == 0).any()
    # afterwards: the evaluation is gone, the parameters are not; the NaN is latched at the next evaluation
    assert np.array_equal(_np(bp.params()), alpha)
    assert bp.residuals() is None
    bp.set_params_with_basis(dev(alpha), dev(Phi_in[:, None, :]), dev(np.zeros((B, 1, m), dtype)))
    if B > 1:
        st = _np(bp.status())
        assert st[NAN_B] != 0 and st[BAD_B] != 0

    # a fixed scale (1.5 is a number of both dtypes): the weights of the mirror at that scale, and the scale echoed
    good, F = _evaluated(bp, dev, Phi_in, Y, w_first, dtype)
    out = bp.robust_reweight(dev(Yn), loss, scale=1.5, base_weights=dev(w0))
    _check_against_mirror(bp, out, Yn, F, w0, loss, 1.5, good, dtype, "fixed scale")
    assert (_np(out[0])[good] == 1.5).all()
    if B > 1:  # the NaN stays in its row
        assert np.isnan(_np(bp.weights())[NAN_B]).sum() == 1

    # no base weights: unit weights, and a tuning constant of the caller's
    good, F = _evaluated(bp, dev, Phi_in, Y, w_first, dtype)
    s, rho = bp.robust_reweight(dev(Y), loss, tuning=2.0)
    w_ref, _yw, s_ref, _u = rc.reweight_mirror(Y, F, None, loss, 2.0, 0.0, dtype)
    assert np.array_equal(_np(s)[good], s_ref[good].astype(np.float64))
    _close(_np(bp.weights())[good], w_ref[good], W_UNITS[loss], np.finfo(dtype).eps, "unit base weights w")
    bp.close()


# ---- 2. geometry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("m", [130, 1025])
def test_a_problem_alone_gives_the_bits_of_the_batch(m, dtype):
    """which wave of which workgroup runs a problem changes nothing: problem b of the B = 37 batch, run alone as B = 1 (the
    first wave of the first workgroup), gives the same w, scale and rho; and two handles with the same input agree"""
    Phi_in, Y, Yn, w0, w_first = _inputs(37, m, dtype)

    def run(rows):
        bp = vp.BatchProblem(vp.ExternalModel(1, 1, [(0, 0)], dtype=dtype), Y[rows], weights=w_first[rows])
        bp.set_params_with_basis(np.ones((len(rows), 1), dtype), Phi_in[rows][:, None, :], np.zeros((len(rows), 1, m), dtype))
        s, rho = bp.robust_reweight(Yn[rows], "cauchy", base_weights=w0[rows])
        got = (s, rho, bp.weights(), bp.weighted_data())
        bp.close()
        return got

    whole, twin = run(np.arange(37)), run(np.arange(37))
    for a, b in zip(whole, twin):
        assert np.array_equal(a, b, equal_nan=True)
    for b in (0, EVEN_B, SIX_B, EQUAL_B, NAN_B, ZEROS_B, 18, 35, 36):
        alone = run(np.array([b]))
        for a, c in zip(whole, alone):
            assert np.array_equal(a[b], c[0], equal_nan=True), b


# ---- 3. vp_weights -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", ["host", "torch"])
@pytest.mark.parametrize("per_problem", [False, True])
def test_weights_returns_what_set_weights_was_given(per_problem, device):
    rng = np.random.default_rng(17)
    B, m = 5, 131
    dev = _dev(device)
    x = np.linspace(0.0, 10.0, m)
    mdl = vp.multi_exponential_model(x, [1.0, 4.0])
    Y = rng.poisson(20.0 * np.exp(-x / 2.0) + 1.0, (B, m)).astype(np.float64)
    w1, w2 = (rng.uniform(0.5, 1.5, (B, m) if per_problem else (m,)) for _ in range(2))
    bp = vp.BatchProblem(mdl, dev(Y), weights=dev(w1))
    assert np.array_equal(_np(bp.weights()), w1)
    bp.set_weights(dev(w2), dev(Y))
    assert np.array_equal(_np(bp.weights()), w2) and tuple(bp.weights().shape) == w2.shape
    bp.close()
    bare = vp.BatchProblem(mdl, dev(Y))
    out = np.zeros((B, m))
    assert bare.lib.vp_weights(bare._h, C.c_void_p(out.ctypes.data)) == _lib.VP_ERR_INVALID
    with pytest.raises(ValueError):
        bare.weights()
    bare.close()
    unit = vp.BatchProblem(mdl, dev(Y), weights="unit")
    assert np.array_equal(_np(unit.weights()), np.ones((B, m))) and np.array_equal(_np(unit.weighted_data()), Y)
    unit.close()


# ---- 4. one re-weighted round against the oracle ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _workload(name):
    return rc.workload(name)


@pytest.mark.parametrize("loss", ["huber", "tukey"])
@pytest.mark.parametrize("name", ["double_exp", "lifetime"])
def test_one_round_against_the_oracle(name, loss):
    """fit, robust_reweight, fit: the second fit against the oracle's fit at the mirror's weights of the DEVICE's best fit,
    from the same start, under the contract of every other fit test (tests/contracts.py EXTFIT, unchanged)"""
    wl = _workload(name)
    bp = vp.BatchProblem(wl.model(), wl.Y, weights=wl.w0, irf=wl.irf)
    a1, _C1, rep1 = bp.fit(wl.guess)
    assert (rep1["termination"] > 0).all()
    F = bp.best_fit()
    s, rho = bp.robust_reweight(wl.Y, loss, base_weights=wl.w0)
    a2, C2, rep2 = bp.fit(a1)
    W, _yw, s_ref, u_ref = rc.reweight_mirror(wl.Y, F, wl.w0, loss, rc.K95[loss], 0.0)
    assert np.array_equal(s, s_ref)
    a_ref, _C_ref, term, nev, obj = pc.oracle_round(wl, W, a1)
    assert (term > 0).all()  # the oracle alone succeeds on every problem: none is excluded
    summary = compare_with_oracle(rep2, a2, (a_ref, term, nev, obj))
    print("%s/%s, one re-weighted round: %s" % (name, loss, summary))
    r_ref, mag = rc.rho_mirror(u_ref, loss, rc.K95[loss])
    assert (np.abs(rho.astype(L) - r_ref) <= rc.rho_bound(wl.Y.shape[1], 2) * np.finfo(np.float64).eps * mag).all()
    bp.close()


# ---- 5. fit_robust end to end ----------------------------------------------------------------------------------------------
# What the device may add to the CPU bound on the normalised score.  A device fit may differ from the oracle's by what the
# existing contract allows: a relative objective difference of EXTFIT["objective_rel_max_max"] at worst and
# EXTFIT["objective_rel_median_max"] in the median.  Around the minimum of a round's weighted least-squares problem the
# objective 1/2 sum omega e^2 rises by 1/2 d^T I d, I = J^T J with J = sqrt(omega) g the weighted Jacobian, g = w0 df/dtheta.
# The gradient at the displaced point is I d, and it is s times the estimating function sum psi g at the round's weights
# (e omega = s psi).  With omega <= 1, sum g_k^2 >= I_kk, and by Cauchy-Schwarz each component of the normalised score is
# |e_k^T I d| / (s sqrt(sum g_k^2)) <= sqrt(d^T I d) / s = sqrt(2 rel objective) / s.  The rounds contract such a
# displacement by the factor the CPU sequences show -- CONTRACTION = 0.6, read off the oracle's sequences in
# tests/test_robust_host.py, not off the device -- so what all earlier rounds leave is at most 1/(1 - 0.6) of one round's.
# objective = the fit's reported 1/2 ||r_w||^2, s = the scale of the returned point.
def _score_allowance(objective, rel, scale):
    return ROBUST_SCORE_BOUND + np.sqrt(2.0 * rel * objective) / scale / (1.0 - CONTRACTION)


@pytest.mark.parametrize("name,device,loss", [("double_exp", "host", "huber"), ("double_exp", "torch", "tukey"),
                                              ("lifetime", "host", "tukey"), ("lifetime", "torch", "huber")])
def test_fit_robust_reaches_the_estimating_equations(name, device, loss):
    wl = _workload(name)
    dev = _dev(device)
    irf = None if wl.irf is None else dev(wl.irf)
    bp = vp.BatchProblem(wl.model(), dev(wl.Y), weights=dev(wl.w0), irf=irf)
    a0, _C0, rep0 = bp.fit(dev(wl.guess))
    plain = rc.parameter_error(wl, _np(a0))
    a, Cc, rep, info = bp.fit_robust(dev(wl.Y), dev(wl.guess), loss, base_weights=dev(wl.w0))
    rep = vp.BatchProblem.report_to_numpy(rep)
    assert (rep["termination"] > 0).all() and info["rounds"] == ROBUST_ROUNDS
    a, Cc, s = _np(a), _np(Cc), _np(info["scale"])
    assert (s > 0).all()
    score = rc.normalised_score(wl, a, Cc, loss)
    worst = _score_allowance(rep["objective"], K.EXTFIT["objective_rel_max_max"], s)
    typical = _score_allowance(np.median(rep["objective"]), K.EXTFIT["objective_rel_median_max"], np.median(s))
    print("%s/%s/%s fit_robust: normalised score max %.2e median %.2e (CPU bound %.0e, allowances %.2e / %.2e)"
          % (name, device, loss, score.max(), np.median(score), ROBUST_SCORE_BOUND, worst.min(), typical))
    assert (score <= worst).all() and np.median(score) <= typical
    # the handle's state is the returned point: statistics and best fit without a further call
    assert np.array_equal(_np(bp.params()), a)
    assert (_np(bp.statistics()["status"]) == 0).all()
    assert np.abs(_np(bp.best_fit()) - pc.best_fit(wl, a, Cc)).max() <= 1e-6 * wl.Y.max()
    assert np.array_equal(_np(bp.weights()), _np(info["weights"]))
    # scale, rho and the weights are those of the returned point: the same chain by hand on a second handle (the kernels are
    # deterministic)
    b2 = vp.BatchProblem(wl.model(), wl.Y, weights=wl.w0, irf=wl.irf)
    a2, C2, _rep2 = b2.fit(wl.guess)
    for _ in range(ROBUST_ROUNDS):
        b2.robust_reweight(wl.Y, loss, base_weights=wl.w0)
        a2, C2, _rep2 = b2.fit(a2)
    assert np.array_equal(a2, a) and np.array_equal(C2, Cc)
    s2, rho2 = b2.robust_reweight(wl.Y, loss, base_weights=wl.w0)
    assert np.array_equal(s2, s) and np.array_equal(rho2, _np(info["rho"])) and np.array_equal(b2.weights(), _np(info["weights"]))
    # ... and the outliers have lost their hold on the parameters
    robust = rc.parameter_error(wl, a)
    print("median relative parameter error %.4f plain, %.4f robust" % (plain, robust))
    assert robust < plain
    b2.close()
    bp.close()


# ---- 6. fp32 -----------------------------------------------------------------------------------------------------------------
def test_fit_robust_fp32():
    """fp32 handle, the double exponential, Huber.  The bound is derived like the fp64 one from the contract the project holds
    fp32 fits to (tests/contracts.py CFG4_ALL): at least same_success_class_min of the fits succeed, the relative objective
    difference is objective_rel_median_max in the median and within 1e-3 on share_objective_within_1e-3_min of them"""
    wl = _workload("double_exp")
    f32 = np.float32
    bp = vp.BatchProblem(wl.model(f32), wl.Y.astype(f32), weights=wl.w0.astype(f32))
    a, Cc, rep, info = bp.fit_robust(wl.Y.astype(f32), wl.guess.astype(f32), "huber", base_weights=wl.w0.astype(f32))
    ok = rep["termination"] > 0
    assert ok.mean() >= K.CFG4_ALL["same_success_class_min"]
    assert a.dtype == f32 and info["weights"].dtype == f32 and info["scale"].dtype == np.float64
    with np.errstate(all="ignore"):
        score = rc.normalised_score(wl, a.astype(np.float64), Cc.astype(np.float64), "huber")[ok]
    obj, s = np.median(rep["objective"][ok]), np.median(info["scale"][ok])
    typical = _score_allowance(obj, K.CFG4_ALL["objective_rel_median_max"], s)
    share = K.CFG4_ALL["share_objective_within_1e-3_min"]
    most = _score_allowance(obj, 1e-3, s)
    print("fp32 fit_robust: %d of %d fits ok, normalised score median %.2e, %.0f %% quantile %.2e (allowances %.2e / %.2e)"
          % (ok.sum(), ok.size, np.median(score), 100 * share, np.quantile(score, share), typical, most))
    assert np.median(score) <= typical and np.quantile(score, share) <= most
    assert np.isfinite(info["scale"][ok]).all() and (info["scale"][ok] > 0).all() and (info["rho"][ok] > 0).all()
    bp.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _state(bp):
    return (np.array(bp.weights()) if bp.weighted else None), np.array(bp.weighted_data())


def _refused(bp, code, call):
    before = _state(bp)
    assert call() == code, bp.lib.vp_last_error()
    after = _state(bp)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before, after) if x is not None)


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
    HUB = _lib.VP_ROBUST_HUBER

    def reweight(bp, Yp, loss=HUB, tuning=0.0, scale=0.0):
        return lambda: lib.vp_robust_reweight(bp._h, Yp, _ptr(w), loss, dbl(tuning), dbl(scale), _ptr(out), None)

    bp = vp.BatchProblem(mdl, Y, weights=w)
    bp.evaluate(alpha)
    _refused(bp, INV, reweight(bp, None))
    for loss in (3, -1):
        _refused(bp, INV, reweight(bp, _ptr(Y), loss=loss))
    for bad in (-1.0, np.inf, -np.inf, np.nan):
        _refused(bp, INV, reweight(bp, _ptr(Y), tuning=bad))
        _refused(bp, INV, reweight(bp, _ptr(Y), scale=bad))
    # ... and none of them cost the evaluation: the call goes through afterwards
    assert reweight(bp, _ptr(Y))() == 0
    # straight after a re-weighting the evaluation is gone, although vp_params answers
    assert np.array_equal(bp.params(), alpha)
    _refused(bp, INV, reweight(bp, _ptr(Y)))
    bp.close()

    # before any parameters are set
    bp = vp.BatchProblem(mdl, Y, weights=w)
    _refused(bp, INV, reweight(bp, _ptr(Y)))
    bp.close()

    # a handle without weights, and one with shared weights
    bp = vp.BatchProblem(mdl, Y)
    bp.evaluate(alpha)
    _refused(bp, INV, reweight(bp, _ptr(Y)))
    assert lib.vp_weights(bp._h, _ptr(np.zeros((B, m)))) == INV
    bp.close()
    bp = vp.BatchProblem(mdl, Y, weights=w[0])
    bp.evaluate(alpha)
    _refused(bp, INV, reweight(bp, _ptr(Y)))
    bp.close()

    # S > 1: weights per right-hand side do not exist
    Y3 = np.stack([Y, Y + 1, Y + 2], 1)
    bp = vp.BatchProblem(mdl, Y3, weights=w)
    bp.evaluate(alpha)
    _refused(bp, UNS, reweight(bp, _ptr(Y3)))
    bp.close()

    # m < n: the handle is padded
    Ys, ws = Y[:, :2].copy(), w[:, :2].copy()
    bp = vp.BatchProblem(vp.multi_exponential_model(x[:2].copy(), [1.0, 4.0]), Ys, weights=ws)
    bp.evaluate(alpha)
    assert np.array_equal(bp.weights(), ws)
    _refused(bp, UNS, lambda: lib.vp_robust_reweight(bp._h, _ptr(Ys), _ptr(ws), HUB, dbl(0.0), dbl(0.0), None, None))
    bp.close()

    # a caller-evaluated handle: a stepped fit in progress, and no columns at the current parameters
    def columns(a):
        a = np.asarray(a)
        Phi = np.stack([np.exp(-x[None] / a[:, :1]), np.exp(-x[None] / a[:, 1:]), np.ones((B, m))], 1)
        return Phi, np.stack([Phi[:, 0] * x / a[:, :1] ** 2, Phi[:, 1] * x / a[:, 1:] ** 2], 1)

    ext = vp.BatchProblem(vp.ExternalModel(3, 2, [(0, 0), (1, 1)]), Y, weights=w)
    ext.fit_begin(alpha)
    assert reweight(ext, _ptr(Y))() == INV
    trial = alpha
    for _ in range(300):
        trial, _want, nact = ext.fit_step_with_basis(*columns(trial))
        if nact == 0:
            break
    a_fit, _Cf, _rf = ext.fit_end()
    _refused(ext, INV, reweight(ext, _ptr(Y)))  # (the fitted point's columns are not known)
    # ... with them it works on a caller-evaluated handle
    Phi, dPhi = columns(a_fit)
    e1 = ext.evaluate_with_basis(a_fit, Phi, dPhi)
    s, _rho = ext.robust_reweight(Y, "huber", base_weights=w)
    s_ref = rc.reweight_mirror(Y, np.einsum("bnm,bn->bm", Phi, e1["C"]), w, "huber", rc.K95["huber"], 0.0)[2]
    assert np.allclose(s, s_ref, rtol=1e-9)
    ext.close()
