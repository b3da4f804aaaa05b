"""GPU tier of box bounds on the nonlinear parameters of device-column fits (vp_set_bounds, VP_FLAG_DEVICE_COLUMNS).
A bounded fit is the unchanged LM iteration on internal parameters u with alpha = g(u) (varpro_amd/bounds.py; on the device
bound_map of varpro_amd/csrc/vp_cols.hpp).  THE CHECKER is the CPU oracle fitting the TRANSFORMED problem: `oracle_problem`
(tests/test_gpu_external.py) driven by closures that evaluate the model at from_internal(u) and scale the derivative columns
by dalpha_du(u), started at to_internal(guess), its result mapped back with from_internal -- compared by
`compare_with_oracle` (tests/test_gpu_extfit.py) under the K.EXTFIT contracts.  Guesses are moved strictly inside the box
(2 % of its width, 0.02 on a one-sided bound): a start ON a bound sits at cos u ~ 6e-17, where the two sin implementations
decide the trajectory.  Every test asserts first that the oracle itself succeeds on >= 95 % of the problems."""
import ctypes
import functools

import numpy as np
import pytest

import contracts as K
import varpro_amd as vp
from varpro_amd import _lib, basis, bounds
from test_gpu_external import oracle_problem, peaks_data, peaks_model
from test_gpu_extfit import compare_with_oracle, oracle_fits
from test_gpu_peak_kinds import dev_peaks_model, report_equal

pytestmark = pytest.mark.gpu
INF = np.inf
WIDE = (np.array([2.0, 0.1, 5.5, 0.1]), np.array([4.0, 2.0, 7.5, INF]))
ACTIVE = (np.array([-INF, 0.1, 5.5, 0.3]), np.array([4.0, 0.6, 7.5, 0.8]))


class Transformed:
    """the caller's model in internal parameters: columns at from_internal(u), derivative columns times dalpha_du(u)"""

    def __init__(self, cm, lo, hi):
        self.cm, self.lo, self.hi, self.x = cm, lo, hi, cm.x
        self.k_of_pair = [k for _j, k in cm.pairs()]

    def shape(self):
        return self.cm.shape()

    def pairs(self):
        return self.cm.pairs()

    def eval_batch(self, u):
        return self.cm.eval_batch(bounds.from_internal(u, self.lo, self.hi))

    def derivs_batch(self, u):
        d = self.cm.derivs_batch(bounds.from_internal(u, self.lo, self.hi))
        return d * bounds.dalpha_du(u, self.lo, self.hi)[:, self.k_of_pair, None]


def inside(guess, lo, hi):
    """guesses strictly inside the box: at least 2 % of its width (0.02 on a one-sided bound) away from every bound"""
    lo, hi = np.broadcast_to(lo, guess.shape), np.broadcast_to(hi, guess.shape)
    margin = np.where(np.isfinite(hi - lo), 0.02 * (hi - lo), 0.02)
    return np.minimum(np.maximum(guess, lo + margin), hi - margin)


def transformed_oracle_fits(cm, Y, guess, lo, hi, w=None):
    """(alpha, termination, n_evals, objective) of the oracle's fits of the transformed problems, alpha mapped back; lo / hi
    (q,) or (B, q)"""
    if np.ndim(lo) == 1:
        a, term, nev, obj = oracle_fits(Transformed(cm, lo, hi), Y, bounds.to_internal(guess, lo, hi), w)
        out = bounds.from_internal(a, lo, hi), term, nev, obj
    else:
        parts = [oracle_fits(Transformed(cm, lo[b], hi[b]), Y[b:b + 1], bounds.to_internal(guess[b:b + 1], lo[b], hi[b]), w)
                 for b in range(Y.shape[0])]
        a, term, nev, obj = (np.concatenate([p[k] for p in parts]) for k in range(4))
        out = bounds.from_internal(a, lo, hi), term, nev, obj
    assert (out[1] > 0).mean() >= 0.95, "the checker itself fails on this data"
    return out


@functools.lru_cache(maxsize=None)
def case(m, weighted=False, box="wide"):
    """data, guesses inside the box and the transformed oracle's fits: computed once, shared, never modified"""
    rng = np.random.default_rng(100 + m)
    B = 48
    x = np.linspace(0.0, 10.0, m)
    cm = peaks_model(x)
    _truth, _c, Y, guess = peaks_data(rng, B, x, noise=1e-2)
    w = (0.5 + rng.random(m)) if weighted else None
    lo, hi = WIDE if box == "wide" else ACTIVE
    guess = inside(guess, lo, hi)
    ref = transformed_oracle_fits(cm, Y, guess, lo, hi, w)
    for arr in (Y, guess) + tuple(ref) + ((w,) if weighted else ()):
        arr.setflags(write=False)
    return x, cm, Y, guess, w, lo, hi, ref


def in_box(a, lo, hi):
    a = np.asarray(a, dtype=np.float64)
    return bool(((a >= lo) & (a <= hi)).all())


# ---- 1. identity ---------------------------------------------------------------------------------------------------------
def test_infinite_bounds_and_cleared_bounds_change_nothing():
    x, _cm, Y, guess, _w, _lo, _hi, _ref = case(200)
    plain = vp.BatchProblem(dev_peaks_model(x), Y)
    a0, C0, rep0 = plain.fit(guess)
    r0 = np.asarray(plain.residuals())
    plain.close()
    bp = vp.BatchProblem(dev_peaks_model(x), Y)
    bp.set_bounds(np.full(4, -INF), np.full(4, INF))  # the bounded kernel with the identity map
    a1, C1, rep1 = bp.fit(guess)
    assert np.array_equal(a0, a1) and np.array_equal(C0, C1) and report_equal(rep0, rep1)
    assert np.array_equal(r0, np.asarray(bp.residuals()))
    bp.set_bounds(None, [INF] * 4)
    a1, C1, rep1 = bp.fit(guess)
    assert np.array_equal(a0, a1) and np.array_equal(C0, C1) and report_equal(rep0, rep1)
    bp.set_bounds(*WIDE)
    a2, _C2, _rep2 = bp.fit(guess)
    assert not np.array_equal(a0, a2)                 # (bounds in force take another path)
    bp.set_bounds(None, None)
    a3, C3, rep3 = bp.fit(guess)
    assert np.array_equal(a0, a3) and np.array_equal(C0, C3) and report_equal(rep0, rep3)
    bp.close()


# ---- 2. a box that contains every optimum -------------------------------------------------------------------------------
# (m = 200: one wave per problem; 1003: element-wise stores of the column kernel; 5000: the rows streamed in blocks)
@pytest.mark.parametrize("m,weighted", [(200, False), (200, True), (1003, False), (5000, False)])
def test_wide_box_matches_the_transformed_oracle(m, weighted):
    x, cm, Y, guess, w, lo, hi, ref = case(m, weighted)
    bp = vp.BatchProblem(dev_peaks_model(x), Y, weights=w)
    bp.set_bounds(lo, hi)
    a, C, rep = bp.fit(guess)
    s = compare_with_oracle(rep, a, ref)
    print("wide box m=%d weighted=%s: %s" % (m, weighted, s))
    assert in_box(a, lo, hi)
    # the returned point is the point of the handle's state: no further call is needed
    assert np.array_equal(np.asarray(bp.params()), a) and np.array_equal(np.asarray(bp.linear_coefficients()), C)
    r = np.asarray(bp.residuals())
    okb = rep["termination"] > 0
    assert (np.abs(0.5 * (r ** 2).sum(1) - rep["objective"])[okb] <= 1e-9 * rep["objective"][okb]).all()
    st = bp.statistics()
    assert (np.asarray(st["status"])[okb] == 0).all() and np.isfinite(np.asarray(st["cov"])[okb]).all()
    bp.close()


# ---- 3. a box that cuts optima off ---------------------------------------------------------------------------------------
def test_active_box_keeps_every_parameter_inside():
    """39 of the 48 unconstrained optima lie outside this box.  Measured on an MI355X against the transformed oracle: the same
    termination code on 48 of 48, objectives to 7.5e-16 (median) / 7.2e-15 (worst) relative, evaluation counts within 3 of
    the oracle's on 0.9583 (46 of 48) on the first run -- the figure asserted below -- and on 48 of 48 since g^-1 of a
    one-sided bound is formed without the square."""
    x, cm, Y, guess, _w, lo, hi, ref = case(200, box="active")
    free = vp.BatchProblem(dev_peaks_model(x), Y)
    a_free, _C, rep_free = free.fit(guess)
    free.close()
    outside = ~((a_free >= lo) & (a_free <= hi)).all(1) & (rep_free["termination"] > 0)
    assert outside.sum() >= 1, "the box cuts nothing off: the test would pass vacuously"
    bp = vp.BatchProblem(dev_peaks_model(x), Y)
    bp.set_bounds(lo, hi)
    a, _C, rep = bp.fit(guess)
    bp.close()
    assert (a >= lo).all() and (a <= hi).all()  # bounds included, no tolerance
    a_ref, term, nev, obj = ref
    ok = term > 0
    assert ((rep["termination"] > 0) == ok).all()
    assert (rep["termination"] == term).all(), "termination reasons differ on %s" % np.nonzero(rep["termination"] != term)[0][:8]
    rel = np.abs(rep["objective"] - obj)[ok] / obj[ok]
    share = float((np.abs(rep["n_evals"] - nev) <= 3).mean())
    print("active box: %d of %d unconstrained optima outside; objective rel median %.3e max %.3e; evaluations within 3 of the "
          "oracle on %.4f" % (outside.sum(), len(outside), np.median(rel), rel.max(), share))
    assert np.median(rel) <= K.EXTFIT["objective_rel_median_max"] and rel.max() <= K.EXTFIT["objective_rel_max_max"]
    # fits that converge ONTO a bound end on xtol with cos u -> 0, where the evaluation count is sensitive to rounding: the
    # share is the measured one minus 0.05 (two problems of 48), never below 0.8
    MEASURED_SHARE = 0.9583  # 46 of 48, first run on an MI355X
    assert share >= max(0.8, MEASURED_SHARE - 0.05), share


# ---- 4. per-problem bounds -----------------------------------------------------------------------------------------------
def test_per_problem_boxes():
    x, cm, Y, guess, _w, _lo, _hi, _ref = case(200)
    half = np.array([1.0, 0.3, 1.0, 0.4])  # wide enough for every optimum (truth within 10 % of the guess)
    lo, hi = guess - half, guess + half  # (B, q), centred on each problem's guess
    assert (lo[:, 1] > 0).all() and (np.ptp(lo, axis=0) > 0).all()
    ref = transformed_oracle_fits(cm, Y, guess, lo, hi)
    bp = vp.BatchProblem(dev_peaks_model(x), Y)
    bp.set_bounds(lo, hi)
    a, _C, rep = bp.fit(guess)
    bp.close()
    assert in_box(a, lo, hi)
    compare_with_oracle(rep, a, ref)


# ---- 5. fp32 and device pointers -----------------------------------------------------------------------------------------
def test_fp32_and_device_pointers():
    """the figures of tests/test_gpu_peak_kinds.py::test_fit_fp32_and_device_pointers"""
    import torch
    rng = np.random.default_rng(41)
    m, B = 600, 64
    x = np.linspace(0.0, 10.0, m)
    cm = peaks_model(x)
    lo, hi = WIDE
    _t, _c, Y, guess = peaks_data(rng, B, x, noise=1e-2)
    guess = inside(guess, lo, hi)
    ref = transformed_oracle_fits(cm, Y, guess, lo, hi)
    host = vp.BatchProblem(dev_peaks_model(x), Y)
    host.set_bounds(lo, hi)
    a, C, rep = host.fit(guess)
    dev = torch.device("cuda:0")
    bp = vp.BatchProblem(dev_peaks_model(x), torch.as_tensor(Y, device=dev))
    bp.set_bounds(lo, hi)
    ad, Cd, repd = bp.fit(torch.as_tensor(guess, device=dev))
    assert np.array_equal(ad.cpu().numpy(), a) and np.array_equal(Cd.cpu().numpy(), C) and report_equal(rep, repd)
    assert np.array_equal(bp.residuals().cpu().numpy(), np.asarray(host.residuals()))
    bp.close()
    host.close()
    bp = vp.BatchProblem(dev_peaks_model(x, np.float32), Y.astype(np.float32))
    bp.set_bounds(lo, hi)
    a32, _C32, rep32 = bp.fit(guess.astype(np.float32))
    bp.close()
    assert a32.dtype == np.float32 and in_box(a32, lo, hi)
    ok = ref[1] > 0
    assert ((rep32["termination"] > 0) == ok).mean() >= 0.9
    both = ok & (rep32["termination"] > 0)
    assert np.median(np.abs(rep32["objective"] - ref[3])[both] / ref[3][both]) <= 1e-3
    assert np.median(np.abs(a32 - ref[0])[both] / np.abs(ref[0])[both]) <= 1e-3


# ---- 6. global fit ---------------------------------------------------------------------------------------------------------
def test_global_fit_of_three_right_hand_sides():
    """the contracts of tests/test_gpu_peak_kinds.py::test_global_fit_of_17_right_hand_sides_and_its_statistics"""
    S = 3
    rng = np.random.default_rng(50 + S)
    B, m = 8, 200
    x = np.linspace(0.0, 10.0, m)
    cm = peaks_model(x)
    lo, hi = WIDE
    truth, _c, _Y1, guess = peaks_data(rng, B, x, noise=1e-2)
    guess = inside(guess, lo, hi)
    Cs = np.stack([rng.uniform(5, 50, (B, S)), rng.uniform(5, 50, (B, S)), rng.uniform(0, 5, (B, S))], 2)
    Y = np.einsum("bsn,bnm->bsm", Cs, cm.eval_batch(truth))
    Y = Y + 1e-2 * np.abs(Y).max(2, keepdims=True) * rng.standard_normal(Y.shape)
    bp = vp.BatchProblem(dev_peaks_model(x), Y)
    bp.set_bounds(lo, hi)
    a1, C1, rep = bp.fit(guess)
    assert np.asarray(C1).shape == (B, S, 3) and in_box(a1, lo, hi)
    tm = Transformed(cm, lo, hi)
    n_ok = 0
    for b in range(B):
        p = oracle_problem(tm, Y[b])
        p.set_params(bounds.to_internal(guess[b], lo, hi))
        r = p.fit()
        assert (rep["termination"][b] > 0) == (r.termination > 0), (b, rep[b], r.termination)
        if r.termination > 0:
            n_ok += 1
            assert abs(rep["objective"][b] - r.objective) <= 1e-6 * r.objective, (b, rep["objective"][b], r.objective)
            assert abs(int(rep["n_evals"][b]) - int(r.n_evals)) <= 4
            a_ref = bounds.from_internal(p.params(), lo, hi)
            assert np.abs(a1[b] - a_ref).max() <= 1e-5 * np.abs(a_ref).max()
            Cr = np.asarray(p.linear_coefficients()).reshape(S, 3)
            assert np.abs(C1[b] - Cr).max() <= 1e-5 * np.abs(Cr).max()
    assert n_ok >= 0.95 * B
    g = bp.global_statistics(want_confidence_sigma=True)
    assert (np.asarray(g["status"]) == 0).all()
    for key in ("cov_alpha", "reduced_chi2", "coef_cov", "coef_alpha_cov", "conf_sigma"):
        assert np.isfinite(np.asarray(g[key])).all(), key
    bp.close()


# ---- 7. VP_FLAG_DEVICE_COLUMNS ---------------------------------------------------------------------------------------------
def double_exponential(x):
    """the builder-made double exponential of the README and the same model in closures for the oracle"""
    mdl = (vp.SeparableModelBuilder(["tau1", "tau2"]).initial_parameters([2.0, 6.5])
           .function(["tau1"], basis.EXP_DECAY).partial_deriv("tau1")
           .function(["tau2"], basis.EXP_DECAY).partial_deriv("tau2")
           .invariant_function(basis.CONST).independent_variable(x).build())
    decay, ddecay = (lambda x, t: np.exp(-x / t)), (lambda x, t: np.exp(-x / t) * x / t ** 2)
    cm = (vp.ClosureModel(["tau1", "tau2"], x).function(["tau1"], decay).partial_deriv("tau1", ddecay)
          .function(["tau2"], decay).partial_deriv("tau2", ddecay).invariant_function(lambda x: np.ones_like(x)))
    return mdl, cm


def test_device_columns_flag_bounds_a_double_exponential():
    """The builder-made double exponential of the README.  The K.EXTFIT contract (evaluation counts within 3) presupposes a
    well-posed problem, as in tests/test_gpu_peak_kinds.py::test_mixed_model_gauss_exponential_tail_linear_baseline: with
    decay times that approach each other or the window, an exponential is nearly a combination of the other columns and the
    trajectory is decided by rounding for ANY route (on the batch of varpro_amd.synth.double_exp_batch -- guesses 30 % off,
    the oracle itself needs up to 77 evaluations and sends a decay time to -2e8 -- the unbounded device-column fit was
    measured within 3 evaluations of the oracle on 0.83 of 48 problems, objectives to 1e-6).  So the decay times are
    separated (tau1 in [0.5, 1.5], tau2 in [3, 6] on a window of 12.5), the guesses 10 % off as in `peaks_data`, and the test
    asserts the precondition on the checker's side -- cond(Phi) < 1e3 at the truth and at the oracle's fitted points, no
    oracle fit beyond 30 evaluations -- before it compares."""
    m, B = 256, 48
    x = np.linspace(0.0, 12.5, m)
    mdl, cm = double_exponential(x)
    rng = np.random.default_rng(70)
    truth = np.stack([rng.uniform(0.5, 1.5, B), rng.uniform(3.0, 6.0, B)], 1)
    c = np.stack([rng.uniform(5, 50, B), rng.uniform(5, 50, B), rng.uniform(0, 5, B)], 1)
    Y = np.einsum("bn,bnm->bm", c, cm.eval_batch(truth))
    Y = Y + 1e-3 * np.abs(Y).max(1, keepdims=True) * rng.standard_normal(Y.shape)
    guess = truth * (1 + rng.uniform(-0.1, 0.1, truth.shape))
    dc = vp.BatchProblem(mdl, Y, device_columns=True)
    with pytest.raises(vp.VarproHipError) as e:  # a device-column handle: the caller-evaluated entries tell
        dc.fit_trace(guess)
    assert e.value.code == _lib.VP_ERR_UNSUPPORTED and "device-column" in str(e.value)
    ref = oracle_fits(cm, Y, guess)
    assert (ref[1] > 0).mean() >= 0.95 and ref[2].max() <= 30
    assert max(np.linalg.cond(P.T) for P in np.concatenate([cm.eval_batch(truth), cm.eval_batch(ref[0])])) < 1e3
    a, _C, rep = dc.fit(guess)
    print("double exponential, device columns, unbounded: %s" % (compare_with_oracle(rep, a, ref),))
    lo, hi = np.array([0.5, 0.5]), np.array([20.0, 20.0])
    g_in = inside(guess, lo, hi)
    ref_b = transformed_oracle_fits(cm, Y, g_in, lo, hi)
    assert ref_b[2].max() <= 30
    dc.set_bounds(lo, hi)
    a, _C, rep = dc.fit(g_in)
    assert in_box(a, lo, hi)
    print("double exponential, device columns, tau in [0.5, 20]: %s" % (compare_with_oracle(rep, a, ref_b),))
    dc.close()
    # without the flag: the in-register kernels, which take no bounds -- and go on fitting as before
    bp = vp.BatchProblem(mdl, Y)
    a0, C0, rep0 = bp.fit(guess)
    with pytest.raises(vp.VarproHipError) as e:
        bp.set_bounds(lo, hi)
    assert e.value.code == _lib.VP_ERR_UNSUPPORTED and "VP_FLAG_DEVICE_COLUMNS" in str(e.value)
    a1, C1, rep1 = bp.fit(guess)
    assert np.array_equal(a0, a1) and np.array_equal(C0, C1) and report_equal(rep0, rep1)
    bp.close()


def test_device_columns_flag_on_the_synthetic_double_exponential_batch():
    """The batch of varpro_amd.synth.double_exp_batch (decay times that may approach each other, guesses 30 % off), on which
    the test above does not rely for the evaluation-count contract: here the OBJECTIVE contracts of K.EXTFIT and the success
    class alone, unbounded against the oracle's ordinary fit and with tau in [0.5, 20] against the transformed oracle, and
    every bounded result inside the box.  The shares of evaluation counts within 3 of the oracle's are printed, not asserted
    (DESIGN.md section 3f has the measured ones)."""
    from varpro_amd import synth
    m, B = 256, 48
    d = synth.double_exp_batch(B, m=m, noise=1e-3)
    x, Y, guess = d["x"], d["Y"], d["tau_guess"]
    mdl, cm = double_exponential(x)
    lo, hi = np.array([0.5, 0.5]), np.array([20.0, 20.0])
    g_in = inside(guess, lo, hi)
    ref = oracle_fits(cm, Y, guess)
    assert (ref[1] > 0).mean() >= 0.95, "the checker itself fails on this data"
    ref_b = transformed_oracle_fits(cm, Y, g_in, lo, hi)
    dc = vp.BatchProblem(mdl, Y, device_columns=True)
    for name, start, want in (("unbounded", guess, ref), ("tau in [0.5, 20]", g_in, ref_b)):
        if want is ref_b:
            dc.set_bounds(lo, hi)
        a, _C, rep = dc.fit(start)
        _a_ref, term, nev, obj = want
        ok = term > 0
        rel = np.abs(rep["objective"] - obj)[ok] / obj[ok]
        print("synthetic double exponential, device columns, %s: objective rel median %.3e max %.3e; evaluations within 3 of "
              "the oracle on %.4f; oracle evaluations up to %d" % (name, np.median(rel), rel.max(),
                                                                   (np.abs(rep["n_evals"] - nev) <= 3).mean(), nev.max()))
        assert ((rep["termination"] > 0) == ok).all(), np.nonzero((rep["termination"] > 0) != ok)[0][:8]
        assert np.median(rel) <= K.EXTFIT["objective_rel_median_max"] and rel.max() <= K.EXTFIT["objective_rel_max_max"]
        if want is ref_b:
            assert in_box(a, lo, hi)
    dc.close()


# ---- 8. refusals and persistence -------------------------------------------------------------------------------------------
def test_refusals_persistence_and_fit_pipeline():
    import torch
    x, _cm, Y, guess, _w, lo, hi, ref = case(200)
    dp = ctypes.POINTER(ctypes.c_double)
    ptr = lambda v: np.ascontiguousarray(v, dtype=np.float64).ctypes.data_as(dp)
    bp = vp.BatchProblem(dev_peaks_model(x), Y)
    bp.set_bounds(lo, hi)
    a, C, rep = bp.fit(guess)
    nan_lo, eq_hi, gt_hi = lo.copy(), hi.copy(), hi.copy()
    nan_lo[2], eq_hi[1], gt_hi[0] = np.nan, lo[1], lo[0] - 1.0
    keep = [nan_lo, eq_hi, gt_hi]
    for lower, upper in ((keep[0], hi), (lo, keep[1]), (lo, keep[2]), (lo, None), (None, hi)):
        rc = bp.lib.vp_set_bounds(bp._h, None if lower is None else ptr(lower), None if upper is None else ptr(upper), 0)
        assert rc == _lib.VP_ERR_INVALID, (lower, upper)
    a1, C1, rep1 = bp.fit(guess)  # a refusal leaves the handle and the bounds it had
    assert np.array_equal(a, a1) and np.array_equal(C, C1) and report_equal(rep, rep1)
    # the bounds survive new observations
    rng = np.random.default_rng(7)
    _t, _c, Y2, g2 = peaks_data(rng, Y.shape[0], x, noise=1e-2)
    g2 = inside(g2, lo, hi)
    fresh = vp.BatchProblem(dev_peaks_model(x), Y2)
    fresh.set_bounds(lo, hi)
    want = fresh.fit(g2)
    fresh.close()
    bp.set_observations(Y2)
    got = bp.fit(g2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and report_equal(got[2], want[2])
    assert in_box(got[0], lo, hi)
    bp.close()
    # throughput mode: every slot's handle has the bounds
    dev = torch.device("cuda:0")
    alo, ahi = ACTIVE
    g3 = inside(np.asarray(guess), alo, ahi)
    Y = np.array(Y)  # (a writable copy: torch refuses read-only arrays)
    pipe = vp.FitPipeline(dev_peaks_model(x), torch.as_tensor(Y, device=dev), n_slots=2, lower=alo, upper=ahi)
    outs = [pipe.submit(torch.as_tensor(Yk, device=dev), torch.as_tensor(g3, device=dev)) for Yk in (Y, Y2, Y)]
    pipe.wait()
    torch.cuda.synchronize()
    for ak, _Ck, _repk, _slot in outs:
        assert in_box(ak.cpu().numpy(), alo, ahi)
    assert np.array_equal(outs[0][0].cpu().numpy(), outs[2][0].cpu().numpy())
    pipe.close()
