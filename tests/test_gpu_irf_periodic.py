"""GPU tier of the periodic IRF reconvolution kind (VP_BASIS_EXP_DECAY_IRF_PERIODIC): irf_cols_periodic_kernel
(varpro_amd/csrc/vp_irf.hpp) runs the scan of kind 9 twice -- a totals pass, then the columns from the steady-state carry.
Columns are checked against the closed-form periodic sums in long double (tests/irf_periodic_cases.py) under the rule of
tests/test_gpu_irf.py, fits against the oracle driven by closures built on the numpy mirror under K.EXTFIT; the
caller-evaluated route, fed with the columns vp_basis returns, must agree BIT FOR BIT."""
import ctypes as C_
import functools

import numpy as np
import pytest

import contracts as K
import irf_cases as ic
import irf_periodic_cases as pc
import search_cases as sc
import varpro_amd as vp
from varpro_amd import basis, bounds
from test_gpu_bounds import inside, transformed_oracle_fits
from test_gpu_extfit import compare_with_oracle, oracle_fits
from test_gpu_peak_kinds import columns_from, report_equal

pytestmark = pytest.mark.gpu
EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
PER = basis.EXP_DECAY_IRF_PERIODIC


# ---- 1. columns ------------------------------------------------------------------------------------------------------
def mixed_model(x, dtype=np.float64):
    """the mixed descriptor of tests/test_gpu_irf.py with periodic decays in place of kind 9: c1 (irf * exp tau1) +
    c2 Gauss(mu, s) + c3 (irf * exp tau2) + c4 irf + c5 (n = 5, q = 4, p = 4; pairs: tau1 | mu, s | tau2)"""
    return (vp.SeparableModelBuilder(["tau1", "mu", "s", "tau2"], dtype=dtype)
            .function(["tau1"], PER).partial_deriv("tau1")
            .function(["mu", "s"], basis.GAUSS).partial_deriv("mu").partial_deriv("s")
            .function(["tau2"], PER).partial_deriv("tau2")
            .invariant_function(basis.IRF).invariant_function(basis.CONST)
            .independent_variable(x).initial_parameters([1.0, 3.0, 0.5, 4.0]).build())


def small_model(x, n, dtype=np.float64):
    """m < 5: the periodic decay alone (n = 1) or with the response (n = 2)"""
    b = vp.SeparableModelBuilder(["tau1"], dtype=dtype).function(["tau1"], PER).partial_deriv("tau1")
    if n == 2:
        b = b.invariant_function(basis.IRF)
    return b.independent_variable(x).initial_parameters([1.0]).build()


def _column_case(m, dtype, per_problem, longer, B=12):
    """grids, responses, lifetimes and the period of one column case.  tau/dt log-spaced over the batch from 2 (fp64) / 8
    (fp32: below, exp(-(T - m dt)/tau) of the longer period leaves the fp32 range and row 0 of the derivative, which is the
    tail alone, has no relative accuracy) to 16 000, tau2 in reverse order.  Per-problem grids differ in step (by at most
    14 %: the period is shared, and the gap of the shortest record must stay inside the range as well) and origin; fp32
    grids are exactly representable (a step of k/128).  longer: period = (1.37 m + 0.5) dt of the longest record, rounded
    to the dtype; else the default, every record one period"""
    rng = np.random.default_rng(2000 + m)
    T = np.dtype(dtype).type
    if dtype == np.float32:
        dts = np.array([(14 + (b % 3 if per_problem else 0)) / 128.0 for b in range(B)])
        t0 = np.array([(b % 3 if per_problem else 0) * 0.25 for b in range(B)])
    else:
        dts = 0.02 * (1 + (0.01 * np.arange(B) if per_problem else np.zeros(B)))
        t0 = 0.3 * np.arange(B) if per_problem else np.zeros(B)
    X = (t0[:, None] + np.arange(m)[None, :] * dts[:, None]).astype(dtype)
    if per_problem:
        irf = np.stack([ic.response(m, centre=c, width=w) for c, w in zip(rng.uniform(0.05, 0.3, B), rng.uniform(0.005, 0.03, B))])
    else:
        irf = ic.response(m)
    irf = irf.astype(dtype)
    ratio = np.geomspace(2.0 if dtype == np.float64 else 8.0, 16000.0, B)
    n = 5 if m >= 5 else m
    if n == 5:
        span = float(dts[0]) * m
        a = np.stack([ratio * dts, t0 + rng.uniform(0.2, 0.8, B) * span, rng.uniform(0.05, 0.2, B) * span, ratio[::-1] * dts], 1)
    else:
        a = (ratio * dts)[:, None]
    period = float(T((1.37 * m + 0.5) * max(float(ic.grid_step(X[b])) for b in range(B)))) if longer else None
    return X, irf, a.astype(dtype), n, period


def _check_columns(m, dtype, per_problem, longer):
    eps = EPS64 if dtype == np.float64 else EPS32
    X, irf, a, n, period = _column_case(m, dtype, per_problem, longer)
    B = X.shape[0]
    x = X if per_problem else X[0]
    mdl = mixed_model(X[0], dtype) if n == 5 else small_model(X[0], n, dtype)
    dc = vp.BatchProblem(mdl, np.zeros((B, m), dtype=dtype), x=x, irf=irf, irf_period=period)
    Phi, dPhi = dc.basis(a)
    Phi_only, _ = dc.basis(a, want_dphi=False)
    _, dPhi_only = dc.basis(a, want_phi=False)
    Phi_skip, _ = dc.basis(a, skip_invariant=True)
    dc.close()
    assert Phi.dtype == dtype and Phi.shape == (B, n, m) and dPhi.shape == (B, 4 if n == 5 else 1, m)
    assert np.array_equal(Phi_only, Phi) and np.array_equal(dPhi_only, dPhi)
    assert np.array_equal(Phi_skip, Phi[:, :4] if n == 5 else Phi)
    decays = [(0, 0, 0), (2, 3, 3)] if n == 5 else [(0, 0, 0)]  # (column of Phi, column of dPhi, parameter)
    dev = ref = 0.0
    for b in range(B):
        v = irf[b] if per_problem else irf
        dt = ic.grid_step(X[b])
        for jc, pcol, k in decays:
            F_n, D_n = pc.mirror(v, dt, a[b, k], period)
            sums = pc.periodic_sums(v, dt, a[b, k], period)
            dev = max(dev, *pc.column_errors(Phi[b, jc], dPhi[b, pcol], v, dt, a[b, k], eps, sums=sums))
            ref = max(ref, *pc.column_errors(F_n, D_n, v, dt, a[b, k], eps, sums=sums))
        if n >= 2:
            assert np.array_equal(Phi[b, 3 if n == 5 else 1], v)
    if n == 5:  # the columns of the other kinds come from the column kernel, untouched
        assert (Phi[:, 4] == 1).all()
        mu, s = a[:, 1:2].astype(np.float64), a[:, 2:3].astype(np.float64)
        X64 = X.astype(np.float64)
        g = np.exp(-0.5 * ((X64 - mu) / s) ** 2)
        tol = 1e-12 if dtype == np.float64 else 2e-4
        assert np.abs(Phi[:, 1] - g).max() <= tol
        assert np.abs(dPhi[:, 1] - g * (X64 - mu) / s ** 2).max() <= tol * np.abs(g * (X64 - mu) / s ** 2).max()
        assert np.abs(dPhi[:, 2] - g * (X64 - mu) ** 2 / s ** 3).max() <= tol * np.abs(g * (X64 - mu) ** 2 / s ** 3).max()
    print("periodic irf columns %s m=%d per_problem=%s longer=%s: device max %.3f, numpy mirror max %.3f [eps (1 + l_i) |value|]"
          % (np.dtype(dtype).name, m, per_problem, longer, dev, ref))
    assert dev <= 2 * ref + 4, (dev, ref)


@pytest.mark.parametrize("longer", [False, True])
@pytest.mark.parametrize("m", [2, 127, 128, 129, 257, 1030])
@pytest.mark.parametrize("per_problem", [False, True])
def test_columns_against_long_double(m, per_problem, longer):
    """vp_basis (fp64) against the periodic sums in long double: one group, either side of a tile edge, the odd unaligned
    case, several tiles with a tail (the row m-1 of the totals pass lies inside a tile and inside a group); the rule of
    tests/test_gpu_irf.py unchanged: device <= 2 x the numpy mirror's error + 4 units, same dtype, same units."""
    _check_columns(m, np.float64, per_problem, longer)


@pytest.mark.parametrize("longer", [False, True])
@pytest.mark.parametrize("m", [255, 256, 257, 602])
@pytest.mark.parametrize("per_problem", [False, True])
def test_columns_fp32_against_long_double(m, per_problem, longer):
    """fp32: tiles of 256 rows, groups of four; the same rule at the rounded fp32 inputs"""
    _check_columns(m, np.float32, per_problem, longer)


# ---- 2. kinds 9 and 11 side by side, the long period ---------------------------------------------------------------------
def _pair_model(x, kinds):
    b = vp.SeparableModelBuilder(["tau%d" % j for j in range(len(kinds))])
    for j, k in enumerate(kinds):
        b = b.function(["tau%d" % j], k).partial_deriv("tau%d" % j)
    return b.invariant_function(basis.IRF).independent_variable(x).initial_parameters([1.0] * len(kinds)).build()


@pytest.mark.parametrize("m", [129, 1030])
def test_kinds_9_and_11_in_one_descriptor(m):
    """the same tau in both: the kind-9 column has the bits of a handle without the periodic kind, and the difference of
    the two columns is the tail rho^(i+1) F_{-1} (long double), in the units of the periodic column"""
    B, dt = 8, 0.02
    x = dt * np.arange(m)
    irf = ic.response(m)
    tau = np.geomspace(2.0, 16000.0, B) * dt
    a = np.stack([tau, tau], 1)
    both = vp.BatchProblem(_pair_model(x, [basis.EXP_DECAY_IRF, PER]), np.zeros((B, m)), irf=irf)
    Phi, dPhi = both.basis(a)
    both.close()
    plain = vp.BatchProblem(_pair_model(x, [basis.EXP_DECAY_IRF]), np.zeros((B, m)), irf=irf)
    Phi9, dPhi9 = plain.basis(tau[:, None])
    plain.close()
    assert np.array_equal(Phi[:, 0], Phi9[:, 0]) and np.array_equal(dPhi[:, 0], dPhi9[:, 0])
    assert np.array_equal(Phi[:, 2], Phi9[:, 1])
    dev = ref = 0.0
    for b in range(B):
        step = ic.grid_step(x)
        Fp, Hp, _G, _s = pc.periodic_sums(irf, step, tau[b])
        Fl, _Hl, _Gl, _sl = ic.direct_sums(irf, step, tau[b])
        tail = Fp - Fl  # == rho^(i+1) F_{-1}
        rho = np.exp(-(ic.L(step) / ic.L(tau[b])))
        assert np.abs(tail - rho ** (np.arange(m) + 1).astype(ic.L) * (tail[0] / rho)).max() <= 4 * m * float(np.finfo(ic.L).eps) * np.abs(Fp).max()  # (rho^k carries k roundings of rho)
        unit = EPS64 * (1 + Hp / Fp) * np.abs(Fp)  # the units of the periodic column, the larger of the two
        diff = Phi[b, 1].astype(ic.L) - Phi[b, 0].astype(ic.L)
        dev = max(dev, float((np.abs(diff - tail) / unit).max()))
        diff_n = pc.mirror(irf, step, tau[b])[0].astype(ic.L) - ic.recurrence(irf, step, tau[b])[0].astype(ic.L)
        ref = max(ref, float((np.abs(diff_n - tail) / unit).max()))
    print("kinds 9 and 11, m=%d: column difference against the tail: device %.3f, numpy %.3f units" % (m, dev, ref))
    assert dev <= 2 * ref + 4, (dev, ref)


def test_a_long_period_gives_the_columns_of_kind_9_bit_for_bit():
    """exp(-T/tau) == 0 in the dtype: the carry is 0 and the second pass is the scan of kind 9"""
    B, m, dt = 6, 257, 0.02
    x = dt * np.arange(m)
    irf = ic.response(m)
    tau = (np.geomspace(2.0, 40.0, B) * dt)[:, None]
    per = vp.BatchProblem(_pair_model(x, [PER]), np.zeros((B, m)), irf=irf, irf_period=800.0 * float(tau.max()))
    Phi, dPhi = per.basis(tau)
    per.close()
    lin = vp.BatchProblem(_pair_model(x, [basis.EXP_DECAY_IRF]), np.zeros((B, m)), irf=irf)
    Phi9, dPhi9 = lin.basis(tau)
    lin.close()
    assert np.array_equal(Phi, Phi9) and np.array_equal(dPhi, dPhi9)


# ---- 3. fits -------------------------------------------------------------------------------------------------------------
SEED = 21  # (the oracle itself converges on all 48 problems of every case below; with seeds 20 and 40 its own first LM step throws
# tau2 of one problem negative -- a property of the reference iteration on that draw, found on the CPU alone)


@functools.lru_cache(maxsize=None)
def _fit_case(m, weighted, S, period_bins):
    """data, closures and the oracle's fits of one case, shared by the tests below (nothing in it is modified)"""
    B = 48
    d = pc.periodic_lifetime_data(SEED + m + S, B, m, S=S, period_bins=period_bins)
    w = (0.5 + np.random.default_rng(3 + m).random(m)) if weighted else None
    cm = pc.periodic_lifetime_closures(d["x"], d["irf"], d["period"])
    ref = oracle_fits(cm, d["Y"], d["guess"], w)
    return d, w, cm, ref


@pytest.mark.parametrize("m,weighted,S,period_bins", [(200, False, 1, None), (1030, False, 1, 1.3 * 1030), (1030, True, 1, None),
                                                      (200, False, 3, None)])
def test_fit_matches_the_oracle_and_the_stepped_fit_bit_for_bit(m, weighted, S, period_bins):
    """The weighted case runs at m = 1030, not 200.  K.EXTFIT allows 2 of 48 evaluation counts to differ from the oracle's
    by more than 3, and at m = 200 with these weights the ORACLE ALONE uses that up: driven by two correct fp64 evaluations
    of the same columns -- the numpy mirror, and the long-double sums rounded to fp64 -- its counts differ by more than 3 on
    2 of 48 problems (4 and 33, by 4 and 5; unweighted: 1 of 48), so the count is decided by the last bit of the columns.
    There the device was within 3 on 45 of 48 (objectives equal to 1e-15 median).  At m = 1030, weighted, both periods, the
    two CPU evaluations agree within 3 on 48 of 48: a case that can tell a wrong kernel from a right one."""
    d, w, cm, ref = _fit_case(m, weighted, S, period_bins)
    assert (ref[1] > 0).all()  # the oracle succeeds on every problem: none is excluded
    dc = vp.BatchProblem(pc.periodic_lifetime_model(d["x"]), d["Y"], weights=w, irf=d["irf"], irf_period=d["period"])
    a, C, rep = dc.fit(d["guess"])
    assert (vp.BatchProblem.report_to_numpy(rep)["termination"] > 0).all()
    s = compare_with_oracle(rep, a, ref)
    print("periodic lifetime fit m=%d weighted=%s S=%d period=%s: %s" % (m, weighted, S, d["period"], s))
    # the stepped fit of an external handle, fed with vp_basis' columns: the same bits
    dc2 = vp.BatchProblem(pc.periodic_lifetime_model(d["x"]), d["Y"], weights=w, irf=d["irf"], irf_period=d["period"])
    ext = vp.BatchProblem(cm.shape(), d["Y"], weights=w)
    a2, C2, rep2, _steps = ext.fit_with_model(columns_from(dc2), d["guess"], check_every=3)
    assert np.array_equal(a, a2) and np.array_equal(C, C2) and report_equal(rep, rep2)
    ext.close()
    dc2.close()
    dc.close()


def test_the_non_periodic_model_fits_the_same_data_worse():
    """kind 9 on incomplete decays: the wrapped tail has nowhere to go but the offset and the long lifetime"""
    d, w, cm, ref = _fit_case(200, False, 1, None)
    per = vp.BatchProblem(pc.periodic_lifetime_model(d["x"]), d["Y"], irf=d["irf"])
    a_p, _C, rep_p = per.fit(d["guess"])
    per.close()
    lin = vp.BatchProblem(ic.lifetime_model(d["x"]), d["Y"], irf=d["irf"])
    a_l, _C, rep_l = lin.fit(d["guess"])
    lin.close()
    obj_p, obj_l = (np.median(vp.BatchProblem.report_to_numpy(r)["objective"]) for r in (rep_p, rep_l))
    err_p, err_l = (np.median(np.abs(np.asarray(a)[:, 1] - d["truth"][:, 1]) / d["truth"][:, 1]) for a in (a_p, a_l))
    print("incomplete decays, m=200: median objective periodic %.4e / kind 9 %.4e; median rel tau2 error periodic %.3e / kind 9 %.3e"
          % (obj_p, obj_l, err_p, err_l))
    assert obj_p < obj_l


def test_bounds():
    """infinite bounds: the bounded periodic kernel with the identity map, the bits of the unbounded fit.  A box in force:
    the oracle on the transformed problem (tau = g(u), derivative columns times dtau/du from varpro_amd.bounds) under
    K.EXTFIT, as tests/test_gpu_bounds.py checks the column kernel's bounded sibling"""
    d, w, cm, ref = _fit_case(200, False, 1, None)
    dc = vp.BatchProblem(pc.periodic_lifetime_model(d["x"]), d["Y"], irf=d["irf"])
    a0, C0, rep0 = dc.fit(d["guess"])
    dc.set_bounds([-np.inf, -np.inf], [np.inf, np.inf])
    a1, C1, rep1 = dc.fit(d["guess"])
    assert np.array_equal(a0, a1) and np.array_equal(C0, C1) and report_equal(rep0, rep1)
    lo, hi = np.array([0.2, 2.0]), np.array([2.0, np.inf])
    guess = inside(d["guess"], lo, hi)
    tref = transformed_oracle_fits(cm, d["Y"], guess, lo, hi)
    dc.set_bounds(lo, hi)
    a2, _C2, rep2 = dc.fit(guess)
    dc.close()
    assert ((a2 >= lo) & (a2 <= hi)).all()
    print("bounded periodic lifetime fit: %s" % compare_with_oracle(rep2, a2, tref))


# ---- 4. search -----------------------------------------------------------------------------------------------------------
def test_search():
    """K = 16 candidates, fp64, a shared response: the winners are numpy's argmin over costs computed from the mirror"""
    B, m = 24, 200
    d = pc.periodic_lifetime_data(77, B, m)
    cand = vp.candidate_grid((0.5, 0.8, 1.1, 1.5), (2.8, 3.7, 4.6, 5.8))
    assert cand.shape == (16, 2)
    cost_np, y2 = pc.periodic_lifetime_costs(d["irf"], d["dt"], cand, d["Y"])
    dc = vp.BatchProblem(pc.periodic_lifetime_model(d["x"]), d["Y"], irf=d["irf"])
    a, idx, cost = dc.search(cand)
    dc.close()
    sc.check_fp64(idx, cost, cost_np, y2, 4, m, 1e-9, cap=0.0)
    assert np.array_equal(idx, cost_np.argmin(1)) and np.array_equal(a, cand[idx])


# ---- 5. state and refusals ---------------------------------------------------------------------------------------------
def test_set_irf_period_on_a_live_handle():
    d, w, cm, ref = _fit_case(200, False, 1, None)
    B, m = d["Y"].shape
    g = d["guess"]
    T2 = 1.5 * m * float(d["dt"])
    dc = vp.BatchProblem(pc.periodic_lifetime_model(d["x"]), d["Y"], irf=d["irf"])
    ev = dc.evaluate(g)
    dc.set_irf_period(T2)
    with pytest.raises(vp.VarproHipError):  # the cached evaluation belongs to the old period
        dc.cost()
    assert not np.array_equal(np.asarray(dc.evaluate(g)["cost"]), np.asarray(ev["cost"]))
    a, C, rep = dc.fit(g)
    fresh = vp.BatchProblem(pc.periodic_lifetime_model(d["x"]), d["Y"], irf=d["irf"], irf_period=T2)
    a2, C2, rep2 = fresh.fit(g)
    fresh.close()
    # (the data belong to the default period: with T2 a few fits end on a non-finite step, their C is NaN in both)
    assert np.array_equal(a, a2, equal_nan=True) and np.array_equal(C, C2, equal_nan=True) and report_equal(rep, rep2)
    assert (vp.BatchProblem.report_to_numpy(rep)["termination"] > 0).mean() >= 0.9
    dc.set_irf_period(None)  # back to one period per record: the first evaluation
    assert np.array_equal(np.asarray(dc.evaluate(g)["cost"]), np.asarray(ev["cost"]))
    # the library's own refusals (the Python layer checks first, so through the C boundary)
    lib = dc.lib
    assert lib.vp_set_irf_period(dc._h, C_.c_double(float("nan"))) == -1
    assert lib.vp_set_irf_period(dc._h, C_.c_double(-1.0)) == -1
    assert lib.vp_set_irf_period(dc._h, C_.c_double(0.9 * m * float(d["dt"]))) == -1
    assert lib.vp_set_irf_period(dc._h, C_.c_double((1 - 5e-7) * m * float(d["dt"]))) == 0  # inside the tolerance: g = 0
    assert np.allclose(np.asarray(dc.evaluate(g)["cost"]), np.asarray(ev["cost"]), rtol=1e-9, atol=0)
    dc.close()
    lin = vp.BatchProblem(ic.lifetime_model(d["x"]), d["Y"], irf=d["irf"])
    assert lin.lib.vp_set_irf_period(lin._h, C_.c_double(T2)) == -1  # a model without the periodic kind
    with pytest.raises(ValueError):
        lin.set_irf_period(T2)
    lin.close()


def test_a_device_grid_with_a_period_shorter_than_the_record_fails_its_problems():
    """device grids are the caller's contract: the kernel answers g < -1e-6 m with NaN columns, latched per problem"""
    import torch
    d, w, cm, ref = _fit_case(200, False, 1, None)
    m = d["Y"].shape[1]
    dev = torch.device("cuda:0")
    tt = lambda v: torch.as_tensor(v, device=dev)  # noqa: E731
    bp = vp.BatchProblem(pc.periodic_lifetime_model(d["x"]), tt(d["Y"]), irf=tt(d["irf"]), irf_period=0.8 * m * float(d["dt"]))
    st = bp.evaluate(tt(d["guess"]))["status"]
    assert (st.cpu().numpy() != 0).all()
    _a, _C, rep = bp.fit(tt(d["guess"]))
    assert (vp.BatchProblem.report_to_numpy(rep)["termination"] < 0).all()
    bp.set_irf_period(None)
    _a, _C, rep = bp.fit(tt(d["guess"]))
    assert (vp.BatchProblem.report_to_numpy(rep)["termination"] > 0).all()
    bp.close()


def test_creation_refuses_the_periodic_kind_on_one_sample():
    x = np.array([0.5])
    mdl = small_model(x, 1)
    desc = mdl.desc()
    lib = vp.load_library()
    h = C_.c_void_p()
    Y = np.zeros((2, 1))
    rc = lib.vp_batch_create(C_.byref(h), C_.byref(desc), 0, 1, 1, 2, C_.c_void_p(x.ctypes.data), C_.c_void_p(Y.ctypes.data),
                             None, -1.0, 0, 0, None)
    assert rc == -1 and not h.value
    with pytest.raises(vp.VarproHipError):
        vp.BatchProblem(mdl, Y, irf=np.ones(1))
