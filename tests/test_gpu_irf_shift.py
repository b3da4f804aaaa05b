"""GPU tier of the shifted IRF kinds (VP_BASIS_EXP_DECAY_IRF_SHIFT, VP_BASIS_IRF_SHIFT, VP_BASIS_EXP_DECAY_IRF_PERIODIC_SHIFT):
the resample kernel (varpro_amd/csrc/vp_irf_shift.hpp) writes the shifted response g and dg/ddelta per problem, and the scan
kernels of kinds 9 - 11 run over them unchanged (launch_irf).  g and g' are checked against the long-double definition
(tests/irf_shift_cases.py) in units of eps (1 + |s|) sum |w_a| |tap|, the reconvolved columns in the sensitivity units of
tests/test_gpu_irf.py fed with the long-double g, both under that file's rule: device <= 2 x the numpy mirror's error + 4
units.  What the routing promises is checked bit for bit.  Fits run against the oracle driven by closures built on the numpy
mirror under K.EXTFIT; the caller-evaluated route, fed with the columns vp_basis returns, must agree BIT FOR BIT."""
import ctypes as C_
import functools

import numpy as np
import pytest

import irf_cases as ic
import irf_periodic_cases as pc
import irf_shift_cases as sh
import varpro_amd as vp
from varpro_amd import basis
from varpro_amd.model import irf_shifted
from test_gpu_bounds import inside, transformed_oracle_fits
from test_gpu_extfit import compare_with_oracle, oracle_fits
from test_gpu_peak_kinds import columns_from, report_equal

pytestmark = pytest.mark.gpu
EPS = {np.float64: float(np.finfo(np.float64).eps), np.float32: float(np.finfo(np.float32).eps)}
S12, S13, S14 = basis.EXP_DECAY_IRF_SHIFT, basis.IRF_SHIFT, basis.EXP_DECAY_IRF_PERIODIC_SHIFT


# ---- 1. columns ------------------------------------------------------------------------------------------------------
def mixed_model(x, dtype=np.float64):
    """every shifted kind next to its unshifted twin and a kind of the column kernel (n = 8, q = 5, p = 9):
    columns  0: 12(tau1, delta)  1: Gauss(mu, s)  2: 14(tau2, delta)  3: 13(delta)  4: 9(tau1)  5: 11(tau2)  6: irf  7: 1
    pairs    0: tau1  1: delta | 2: mu  3: s | 4: tau2  5: delta | 6: delta | 7: tau1 | 8: tau2"""
    return (vp.SeparableModelBuilder(["tau1", "mu", "s", "tau2", "delta"], dtype=dtype)
            .function(["tau1", "delta"], S12).partial_deriv("tau1").partial_deriv("delta")
            .function(["mu", "s"], basis.GAUSS).partial_deriv("mu").partial_deriv("s")
            .function(["tau2", "delta"], S14).partial_deriv("tau2").partial_deriv("delta")
            .function(["delta"], S13).partial_deriv("delta")
            .function(["tau1"], basis.EXP_DECAY_IRF).partial_deriv("tau1")
            .function(["tau2"], basis.EXP_DECAY_IRF_PERIODIC).partial_deriv("tau2")
            .invariant_function(basis.IRF).invariant_function(basis.CONST)
            .independent_variable(x).initial_parameters([1.0, 3.0, 0.5, 4.0, 0.0]).build())


def small_model(x, dtype=np.float64):
    """m = 2: the shifted decay and the shifted response (n = 2; pairs 0: tau1, 1: delta | 2: delta)"""
    return (vp.SeparableModelBuilder(["tau1", "delta"], dtype=dtype)
            .function(["tau1", "delta"], S12).partial_deriv("tau1").partial_deriv("delta")
            .function(["delta"], S13).partial_deriv("delta")
            .independent_variable(x).initial_parameters([1.0, 0.0]).build())


def twin_model(x, dtype=np.float64):
    """kinds 9 and 11 alone: what the derivative pass runs over g'"""
    return (vp.SeparableModelBuilder(["tau1", "tau2"], dtype=dtype)
            .function(["tau1"], basis.EXP_DECAY_IRF).partial_deriv("tau1")
            .function(["tau2"], basis.EXP_DECAY_IRF_PERIODIC).partial_deriv("tau2")
            .independent_variable(x).initial_parameters([1.0, 4.0]).build())


def _shifts(m):
    return [0.0, 0.37, -2.6, 3.0, float(m + 5)]  # bins, one per problem


def _column_case(m, dtype, per_problem):
    """B = 5 problems, one per shift.  Every step has a short mantissa (k/256, fp32: k/128) and the grids are exact in the
    dtype, so an integer number of bins is an exact delta and an exact quotient delta/dt: reference, mirror and device take
    the same stencil there.  Per-problem grids differ in step and origin, per-problem responses in centre and width."""
    B = 5
    rng = np.random.default_rng(3000 + m)
    T = np.dtype(dtype).type
    if dtype == np.float32:
        dts = np.array([(14 + (b % 3 if per_problem else 0)) / 128.0 for b in range(B)])
    else:
        dts = np.array([(5 + (b if per_problem else 0)) / 256.0 for b in range(B)])
    t0 = np.array([(b if per_problem else 0) * 0.25 for b in range(B)])
    X = (t0[:, None] + np.arange(m)[None, :] * dts[:, None]).astype(dtype)
    assert np.array_equal(X.astype(np.float64), t0[:, None] + np.arange(m)[None, :] * dts[:, None])
    if per_problem:
        irf = np.stack([ic.response(m, centre=c, width=w) for c, w in zip(rng.uniform(0.05, 0.3, B), rng.uniform(0.01, 0.03, B))])
    else:
        irf = ic.response(m, 0.12, 0.02)
    irf = irf.astype(dtype)
    ratio = np.geomspace(8.0, 400.0, B)  # tau/dt
    delta = np.array([T(s) * T(dt) for s, dt in zip(_shifts(m), dts)])
    span = dts * m
    if m >= 8:
        a = np.stack([ratio * dts, t0 + rng.uniform(0.2, 0.8, B) * span, rng.uniform(0.05, 0.2, B) * span, ratio[::-1] * dts, delta], 1)
    else:
        a = np.stack([ratio * dts, delta], 1)
    return X, irf, a.astype(dtype)


def _check_columns(m, dtype, per_problem):
    eps = EPS[dtype]
    X, irf, a = _column_case(m, dtype, per_problem)
    B = X.shape[0]
    big = m >= 8
    x = X if per_problem else X[0]
    mdl = mixed_model(X[0], dtype) if big else small_model(X[0], dtype)
    dc = vp.BatchProblem(mdl, np.zeros((B, m), dtype=dtype), x=x, irf=irf)
    Phi, dPhi = dc.basis(a)
    Phi_only, _ = dc.basis(a, want_dphi=False)
    _, dPhi_only = dc.basis(a, want_phi=False)
    Phi_skip, _ = dc.basis(a, skip_invariant=True)
    a0 = a.copy()
    a0[:, -1] = 0
    Phi0, dPhi0 = dc.basis(a0)
    dc.close()
    n, p = (8, 9) if big else (2, 3)
    assert Phi.dtype == dtype and Phi.shape == (B, n, m) and dPhi.shape == (B, p, m)
    assert np.array_equal(Phi_only, Phi) and np.array_equal(dPhi_only, dPhi)
    assert np.array_equal(Phi_skip, Phi[:, :7] if big else Phi)
    jg, pg = (3, 6) if big else (1, 2)  # where g and g' come out: the column and the pair of the kind-13 function
    # (a) delta = 0: the shifted kinds have the bits of their unshifted twins on the same handle
    rsp = irf if per_problem else np.broadcast_to(irf, (B, m))
    assert np.array_equal(Phi0[:, jg], rsp)
    if big:
        assert np.array_equal(Phi0[:, 0], Phi0[:, 4]) and np.array_equal(dPhi0[:, 0], dPhi0[:, 7])
        assert np.array_equal(Phi0[:, 2], Phi0[:, 5]) and np.array_equal(dPhi0[:, 4], dPhi0[:, 8])
        assert np.array_equal(Phi0[:, 6], rsp) and np.array_equal(Phi[:, 6], rsp) and (Phi[:, 7] == 1).all()
        # ... and the unshifted kinds do not see the shift
        assert np.array_equal(Phi[:, 4:6], Phi0[:, 4:6]) and np.array_equal(dPhi[:, 7:9], dPhi0[:, 7:9])
        assert np.array_equal(Phi[:, 1], Phi0[:, 1]) and np.array_equal(dPhi[:, 2:4], dPhi0[:, 2:4])
    # (b) the derivative pass: the delta column of kinds 12 and 14 is the Phi column kinds 9 and 11 give on g'
    gp = np.ascontiguousarray(dPhi[:, pg])
    if big:
        tw = vp.BatchProblem(twin_model(X[0], dtype), np.zeros((B, m), dtype=dtype), x=x, irf=gp)
        PhiT, _ = tw.basis(np.ascontiguousarray(a[:, [0, 3]]))
        tw.close()
        assert np.array_equal(dPhi[:, 1], PhiT[:, 0]) and np.array_equal(dPhi[:, 5], PhiT[:, 1])
    # (c) the shift beyond the record: exact zeros in everything that reads g or g'
    assert (Phi[4, jg] == 0).all() and (dPhi[4, pg] == 0).all() and (Phi[4, 0] == 0).all() and (dPhi[4, :2] == 0).all()
    # (d) g, g' and the reconvolved columns against long double
    dev = ref = dev_c = ref_c = 0.0
    for b in range(B):
        v = irf[b] if per_problem else irf
        dt = ic.grid_step(X[b])
        delta = a[b, -1]
        lng = sh.shifted_long_double(v, dt, delta)
        g_n, dg_n = irf_shifted(v, dt, delta)
        dev = max(dev, *sh.shift_errors(Phi[b, jg], dPhi[b, pg], v, dt, delta, eps, lng))
        ref = max(ref, *sh.shift_errors(g_n, dg_n, v, dt, delta, eps, lng))
        decays = [(0, 0, 0, None), (2, 4, 3, 0.0)] if big else [(0, 0, 0, None)]  # (column, pair of tau, parameter, period)
        for jc, pcol, k, per in decays:
            F_n, D_n = vp.model.irf_columns(g_n, dt, a[b, k], per)
            if per is None:
                sums = ic.direct_sums(lng[0], dt, a[b, k])
            else:
                sums = pc.periodic_sums(lng[0], dt, a[b, k])
            with np.errstate(all="ignore"):
                dev_c = max(dev_c, *ic.column_errors(Phi[b, jc], dPhi[b, pcol], None, dt, a[b, k], eps, sums=sums))
                ref_c = max(ref_c, *ic.column_errors(F_n, D_n, None, dt, a[b, k], eps, sums=sums))
    print("shifted irf %s m=%d per_problem=%s: g / g' device max %.3f, numpy mirror max %.3f [eps (1 + |s|) sum |w| |tap|]; "
          "columns of kinds 12 / 14 device max %.3f, mirror max %.3f [eps (1 + l_i) |value|]"
          % (np.dtype(dtype).name, m, per_problem, dev, ref, dev_c, ref_c))
    assert dev <= 2 * ref + 4, (dev, ref)
    assert dev_c <= 2 * ref_c + 4, (dev_c, ref_c)
    return dev, ref, dev_c, ref_c  # (tools/irf_shift_probe.py records them)


@pytest.mark.parametrize("m", [2, 127, 128, 129, 257, 1030])
@pytest.mark.parametrize("per_problem", [False, True])
def test_columns_fp64(m, per_problem):
    """one group, either side of a scan tile, the odd unaligned case, several tiles, and 1030: past the 512-row piece of a
    workgroup of the resample kernel and longer than a scan tile"""
    _check_columns(m, np.float64, per_problem)


@pytest.mark.parametrize("m", [255, 256, 257, 1030])
@pytest.mark.parametrize("per_problem", [False, True])
def test_columns_fp32(m, per_problem):
    """fp32: groups of four (1030 is no multiple), tiles of 256 rows, pieces of 1024"""
    _check_columns(m, np.float32, per_problem)


@pytest.mark.parametrize("dtype,m", [(np.float64, 129), (np.float64, 1030), (np.float32, 258)])
def test_integer_shifts_move_the_response_bit_for_bit(dtype, m):
    """dt = 0.25: delta/dt is exact, f = 0, w = (0, 1, 0, 0): vp_basis of a kind-13 function returns the moved samples with
    zeros shifted in"""
    ks = [1, 3, -2, -7, m - 1, -(m - 1)]
    B = len(ks)
    x = (0.25 * np.arange(m)).astype(dtype)
    irf = (ic.response(m, 0.3, 0.04) * np.random.default_rng(m).uniform(0.5, 1.5, m)).astype(dtype)
    mdl = (vp.SeparableModelBuilder(["delta"], dtype=dtype).function(["delta"], S13).partial_deriv("delta")
           .independent_variable(x).initial_parameters([0.0]).build())
    dc = vp.BatchProblem(mdl, np.zeros((B, m), dtype=dtype), irf=irf)
    Phi, _ = dc.basis(np.array([[0.25 * k] for k in ks], dtype=dtype))
    dc.close()
    for b, k in enumerate(ks):
        want = np.zeros(m, dtype)
        if k > 0:
            want[k:] = irf[:m - k]
        else:
            want[:m + k] = irf[-k:]
        assert np.array_equal(Phi[b, 0], want), k


# ---- 2. fits ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fit_case(seed, m, kind=S12, scatter=False, weighted=False, S=1):
    """data, closures and the oracle's fits of one case, shared by the tests below (nothing in it is modified).  The random
    stream is seeded with seed + m + S, as tests/test_gpu_irf_periodic.py seeds its cases."""
    B = 48
    d = sh.shifted_data(seed + m + S, B, m, kind=kind, scatter=scatter, S=S)
    w = (0.5 + np.random.default_rng(3 + m).random(m)) if weighted else None
    cm = sh.shifted_closures(d["x"], d["irf"], kind, scatter)
    ref = oracle_fits(cm, d["Y"], d["guess"], w)
    return d, w, cm, ref


@pytest.mark.parametrize("seed,m,kind,weighted,S", [(21, 200, S12, False, 1), (22, 200, S12, False, 1), (21, 1030, S12, False, 1),
                                                    (22, 1030, S12, False, 1), (21, 200, S14, False, 1), (21, 1030, S12, True, 1),
                                                    (21, 200, S12, False, 3)])
def test_fit_matches_the_oracle_and_the_stepped_fit_bit_for_bit(seed, m, kind, weighted, S):
    """the scatter-free model (two shifted decays + constant: n = 3, q = 3, p = 4), on which the evaluation-count contract of
    K.EXTFIT is asserted: checked on the CPU, the oracle succeeds on 48 of 48 problems of every case here (asserted below; the
    periodic case with seed 22 is not among them: one of its oracle fits fails), needs at most 17 evaluations (S = 1) and
    recovers delta to 0.04 - 0.08 bin in the median."""
    d, w, cm, ref = _fit_case(seed, m, kind, False, weighted, S)
    assert (ref[1] > 0).all()  # the oracle succeeds on every problem: none is excluded
    dc = vp.BatchProblem(sh.shifted_model(d["x"], kind), d["Y"], weights=w, irf=d["irf"])
    a, C, rep = dc.fit(d["guess"])
    assert (vp.BatchProblem.report_to_numpy(rep)["termination"] > 0).all()
    s = compare_with_oracle(rep, a, ref)
    err = np.abs(np.asarray(a)[:, 2] - d["truth"][:, 2]) / d["dt"]
    print("shifted lifetime fit seed=%d m=%d kind=%d weighted=%s S=%d: %s; median |delta error| %.3f bin"
          % (seed, m, kind, weighted, S, s, np.median(err)))
    # the stepped fit of an external handle, fed with vp_basis' columns: the same bits
    dc2 = vp.BatchProblem(sh.shifted_model(d["x"], kind), d["Y"], weights=w, irf=d["irf"])
    ext = vp.BatchProblem(cm.shape(), d["Y"], weights=w)
    a2, C2, rep2, _steps = ext.fit_with_model(columns_from(dc2), d["guess"], check_every=3)
    assert np.array_equal(a, a2) and np.array_equal(C, C2) and report_equal(rep, rep2)
    ext.close()
    dc2.close()
    dc.close()


def test_fit_of_the_full_model_with_the_shifted_scatter_term():
    """n = 4, q = 3, p = 5: the scatter term c3 g makes delta and c3 ill-separated; the oracle succeeds on all 48 but needs
    up to 219 evaluations, and the count is decided by rounding.  As for the ill-separated batch of DESIGN.md section 3f, the
    success class and the two objective limits of K.EXTFIT are asserted, not the counts."""
    d, w, cm, ref = _fit_case(21, 200, S12, True)
    assert (ref[1] > 0).all()
    dc = vp.BatchProblem(sh.shifted_model(d["x"], S12, scatter=True), d["Y"], irf=d["irf"])
    a, C, rep = dc.fit(d["guess"])
    dc.close()
    s = compare_with_oracle(rep, a, ref, evals_share=0.0)
    print("full shifted lifetime fit: %s; oracle evaluations up to %d" % (s, ref[2].max()))


def test_the_unshifted_model_fits_the_same_data_worse():
    d, w, cm, ref = _fit_case(21, 200)
    sft = vp.BatchProblem(sh.shifted_model(d["x"]), d["Y"], irf=d["irf"])
    a_s, _C, rep_s = sft.fit(d["guess"])
    sft.close()
    lin = vp.BatchProblem(sh.unshifted_model(d["x"]), d["Y"], irf=d["irf"])
    a_l, _C, rep_l = lin.fit(d["guess"][:, :2])
    lin.close()
    obj_s, obj_l = (np.median(vp.BatchProblem.report_to_numpy(r)["objective"]) for r in (rep_s, rep_l))
    err_s, err_l = (np.median(np.abs(np.asarray(a)[:, 0] - d["truth"][:, 0]) / d["truth"][:, 0]) for a in (a_s, a_l))
    print("shifted data, m=200: median objective shifted %.4e / kind 9 %.4e; median rel tau1 error shifted %.3e / kind 9 %.3e"
          % (obj_s, obj_l, err_s, err_l))
    assert obj_s < obj_l and err_s < err_l


def test_bounds():
    """delta in [-2 dt, 2 dt] and boxes on the lifetimes: the oracle on the transformed problem under K.EXTFIT, as
    tests/test_gpu_bounds.py checks the column kernel's bounded sibling; dg/ddelta carries ddelta/du from the resample kernel"""
    d, w, cm, ref = _fit_case(21, 200)
    dt = float(d["dt"])
    dc = vp.BatchProblem(sh.shifted_model(d["x"]), d["Y"], irf=d["irf"])
    a0, C0, rep0 = dc.fit(d["guess"])
    dc.set_bounds([-np.inf] * 3, [np.inf] * 3)
    a1, C1, rep1 = dc.fit(d["guess"])
    assert np.array_equal(a0, a1) and np.array_equal(C0, C1) and report_equal(rep0, rep1)
    lo, hi = np.array([0.2, 2.0, -2 * dt]), np.array([2.0, np.inf, 2 * dt])
    guess = inside(d["guess"], lo, hi)
    tref = transformed_oracle_fits(cm, d["Y"], guess, lo, hi)
    dc.set_bounds(lo, hi)
    a2, _C2, rep2 = dc.fit(guess)
    dc.close()
    assert ((a2 >= lo) & (a2 <= hi)).all()
    print("bounded shifted lifetime fit: %s" % compare_with_oracle(rep2, a2, tref))


def test_fixed_delta():
    """fixed={"delta": 0.0}: the kind-9 model on the same handle data, bit for bit in alpha (free part), C and report.  delta
    given per problem: the lifetimes agree with the oracle on kind-9 closures over the mirror's g(delta_b)"""
    d, w, cm, ref = _fit_case(21, 200)
    B = d["Y"].shape[0]
    fx = vp.BatchProblem(sh.shifted_model(d["x"]), d["Y"], irf=d["irf"], fixed={"delta": 0.0})
    a, C, rep = fx.fit(d["guess"])
    lin = vp.BatchProblem(sh.unshifted_model(d["x"]), d["Y"], irf=d["irf"])
    a9, C9, rep9 = lin.fit(d["guess"][:, :2])
    lin.close()
    assert np.array_equal(np.asarray(a)[:, :2], a9) and (np.asarray(a)[:, 2] == 0).all()
    # (the data are shifted: a few of these fits end on a non-finite step, their C is NaN in both)
    assert np.array_equal(C, C9, equal_nan=True) and report_equal(rep, rep9)
    assert (vp.BatchProblem.report_to_numpy(rep)["termination"] > 0).mean() >= 0.9
    delta = d["truth"][:, 2].copy()
    fx.set_fixed(delta=delta)
    a, C, rep = fx.fit(d["guess"])
    fx.close()
    assert np.array_equal(np.asarray(a)[:, 2], delta)
    parts = [oracle_fits(sh.unshifted_closures(d["x"], irf_shifted(d["irf"], d["dt"], delta[b])[0]), d["Y"][b:b + 1], d["guess"][b:b + 1, :2])
             for b in range(B)]
    oref = tuple(np.concatenate([p[k] for p in parts]) for k in range(4))
    assert (oref[1] > 0).all()
    print("fixed shift per problem: %s" % compare_with_oracle(rep, np.asarray(a)[:, :2], oref))


def test_search():
    """K = 12 candidates (tau1, tau2, delta), B = 6: a handle with a shifted kind takes the candidate loop; the winners are
    numpy's argmin over costs computed from the mirror wherever best and second differ by more than 1e-9, relative"""
    d, w, cm, ref = _fit_case(21, 200)
    B = 6
    Y = np.ascontiguousarray(d["Y"][:B])
    dt = float(d["dt"])
    cand = np.array([(t1, t2, s * dt) for t1 in (0.7, 1.3) for t2 in (3.5, 5.0) for s in (-1.0, 0.0, 1.0)])
    assert cand.shape == (12, 3)
    cost_np, _y2 = sh.model_costs(d["irf"], d["dt"], cand, Y)
    dc = vp.BatchProblem(sh.shifted_model(d["x"]), Y, irf=d["irf"])
    a, idx, cost = dc.search(cand)
    dc.close()
    srt = np.sort(cost_np, 1)
    decided = (srt[:, 1] - srt[:, 0]) > 1e-9 * srt[:, 0]
    assert decided.any()
    assert np.array_equal(np.asarray(idx)[decided], cost_np.argmin(1)[decided]) and np.array_equal(a, cand[np.asarray(idx)])
    chosen = cost_np[np.arange(B), np.asarray(idx)]
    assert np.allclose(np.asarray(cost), chosen, rtol=1e-9, atol=0)


# ---- 3. refusals -----------------------------------------------------------------------------------------------------
def test_refusals():
    lib = vp.load_library()
    # one sample: dt = 0
    x1 = np.array([0.5])
    m1 = (vp.SeparableModelBuilder(["delta"]).function(["delta"], S13).partial_deriv("delta")
          .independent_variable(x1).initial_parameters([0.0]).build())
    h = C_.c_void_p()
    Y1 = np.zeros((2, 1))
    rc = lib.vp_batch_create(C_.byref(h), C_.byref(m1.desc()), 0, 1, 1, 2, C_.c_void_p(x1.ctypes.data), C_.c_void_p(Y1.ctypes.data),
                             None, -1.0, 0, 0, None)
    assert rc == -1 and not h.value
    # two different shifts, and a shift that another kind reads (the builder refuses both: through the C boundary)
    d, w, cm, ref = _fit_case(21, 200)
    B, m = d["Y"].shape
    for second in ((S12, 0, 1), (basis.EXP_DECAY, 2, -1)):  # (tau2 as a second delta; exp(-t/delta))
        desc = sh.shifted_model(d["x"]).desc()
        desc.kind[1] = second[0]
        desc.param[1][0], desc.param[1][1] = second[1], second[2]
        rc = lib.vp_batch_create(C_.byref(h), C_.byref(desc), 0, m, 1, B, C_.c_void_p(d["x"].ctypes.data),
                                 C_.c_void_p(d["Y"].ctypes.data), None, -1.0, 0, 0, None)
        assert rc == -1 and not h.value
    # no response yet
    dc = vp.BatchProblem(sh.shifted_model(d["x"]), d["Y"])
    with pytest.raises(vp.VarproHipError):
        dc.fit(d["guess"])
    dc.set_irf(d["irf"])
    # a NaN shift latches its own problem only
    g = d["guess"].copy()
    g[5, 2] = np.nan
    st = np.asarray(dc.evaluate(g)["status"])
    assert st[5] != 0 and (np.delete(st, 5) == 0).all()
    _a, _C, rep = dc.fit(g)
    term = vp.BatchProblem.report_to_numpy(rep)["termination"]
    assert term[5] < 0 and (np.delete(term, 5) > 0).all()
    dc.close()
