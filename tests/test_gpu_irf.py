"""GPU tier of the IRF reconvolution kinds (VP_BASIS_EXP_DECAY_IRF, VP_BASIS_IRF): the scan kernel
(varpro_amd/csrc/vp_irf.hpp) fills their columns of a device-column handle, the column kernel every other kind's, and the
kernels of caller-evaluated models do everything downstream.  Columns are checked against the defining sums in long double,
fits against the oracle driven by closures built on the sequential recurrence (tests/irf_cases.py) under K.EXTFIT; the
caller-evaluated route, fed with the columns vp_basis returns, must agree BIT FOR BIT."""
import functools

import numpy as np
import pytest

import contracts as K
import irf_cases as ic
import search_cases as sc
import varpro_amd as vp
from varpro_amd import basis
from test_gpu_extfit import compare_with_oracle, oracle_fits
from test_gpu_peak_kinds import columns_from, report_equal

pytestmark = pytest.mark.gpu
EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)


# ---- 1. columns ------------------------------------------------------------------------------------------------------
def mixed_model(x, dtype=np.float64):
    """c1 (irf * exp tau1) + c2 Gauss(mu, s) + c3 (irf * exp tau2) + c4 irf + c5: the IRF kinds around a peak kind -- the
    column kernel's descriptor is cut in two (n = 5, q = 4, p = 4; pairs: tau1 | mu, s | tau2)"""
    return (vp.SeparableModelBuilder(["tau1", "mu", "s", "tau2"], dtype=dtype)
            .function(["tau1"], basis.EXP_DECAY_IRF).partial_deriv("tau1")
            .function(["mu", "s"], basis.GAUSS).partial_deriv("mu").partial_deriv("s")
            .function(["tau2"], basis.EXP_DECAY_IRF).partial_deriv("tau2")
            .invariant_function(basis.IRF).invariant_function(basis.CONST)
            .independent_variable(x).initial_parameters([1.0, 3.0, 0.5, 4.0]).build())


def small_model(x, n, dtype=np.float64):
    """m < 5: the decay alone (n = 1) or the decay and the response (n = 2)"""
    b = vp.SeparableModelBuilder(["tau1"], dtype=dtype).function(["tau1"], basis.EXP_DECAY_IRF).partial_deriv("tau1")
    if n == 2:
        b = b.invariant_function(basis.IRF)
    return b.independent_variable(x).initial_parameters([1.0]).build()


def _column_case(m, dtype, per_problem, B=12):
    """grids, responses and lifetimes of one column case: tau/dt log-spaced from 2 to 16 000 over the batch (tau2 in reverse
    order).  Per-problem grids differ in their step and their origin; fp32 grids are exactly representable (a step of k/128),
    so that the rounded grid is uniform"""
    rng = np.random.default_rng(1000 + m)
    T = np.dtype(dtype).type
    if dtype == np.float32:
        dts = np.array([(3 + (b % 5 if per_problem else 0)) / 128.0 for b in range(B)])
        t0 = np.array([(b % 3 if per_problem else 0) * 0.25 for b in range(B)])
    else:
        dts = 0.02 * (1 + (0.1 * np.arange(B) if per_problem else np.zeros(B)))
        t0 = 0.3 * np.arange(B) if per_problem else np.zeros(B)
    X = (t0[:, None] + np.arange(m)[None, :] * dts[:, None]).astype(dtype)
    if per_problem:
        irf = np.stack([ic.response(m, centre=c, width=w) for c, w in zip(rng.uniform(0.05, 0.3, B), rng.uniform(0.005, 0.03, B))])
    else:
        irf = ic.response(m)
    irf = irf.astype(dtype)
    ratio = np.geomspace(2.0, 16000.0, B)
    n = 5 if m >= 5 else m
    if n == 5:
        span = float(dts[0]) * m
        a = np.stack([ratio * dts, t0 + rng.uniform(0.2, 0.8, B) * span, rng.uniform(0.05, 0.2, B) * span, ratio[::-1] * dts], 1)
    else:
        a = (ratio * dts)[:, None]
    return X, irf, a.astype(dtype), n, T


def _check_columns(m, dtype, per_problem):
    eps = EPS64 if dtype == np.float64 else EPS32
    X, irf, a, n, T = _column_case(m, dtype, per_problem)
    B = X.shape[0]
    x = X if per_problem else X[0]
    mdl = mixed_model(X[0], dtype) if n == 5 else small_model(X[0], n, dtype)
    dc = vp.BatchProblem(mdl, np.zeros((B, m), dtype=dtype), x=x, irf=irf)
    Phi, dPhi = dc.basis(a)
    Phi_only, _ = dc.basis(a, want_dphi=False)
    _, dPhi_only = dc.basis(a, want_phi=False)
    Phi_skip, _ = dc.basis(a, skip_invariant=True)
    dc.close()
    assert Phi.dtype == dtype and Phi.shape == (B, n, m) and dPhi.shape == (B, 4 if n == 5 else 1, m)
    # phi == nullptr / dphi == nullptr / skip_invariant: the same columns
    assert np.array_equal(Phi_only, Phi) and np.array_equal(dPhi_only, dPhi)
    assert np.array_equal(Phi_skip, Phi[:, :4] if n == 5 else Phi)
    decays = [(0, 0, 0), (2, 3, 3)] if n == 5 else [(0, 0, 0)]  # (column of Phi, column of dPhi, parameter)
    dev = ref = 0.0
    for b in range(B):
        v = irf[b] if per_problem else irf
        dt = ic.grid_step(X[b])
        for jc, pc, k in decays:
            F_n, _H, D_n = ic.recurrence(v, dt, a[b, k])
            sums = ic.direct_sums(v, dt, a[b, k])
            dev = max(dev, *ic.column_errors(Phi[b, jc], dPhi[b, pc], v, dt, a[b, k], eps, sums))
            ref = max(ref, *ic.column_errors(F_n, D_n, v, dt, a[b, k], eps, sums))
        # 2. the response column is the response, bit for bit
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
    print("irf columns %s m=%d per_problem=%s: device max %.3f, numpy recurrence max %.3f [eps (1 + l_i) |value|]"
          % (np.dtype(dtype).name, m, per_problem, dev, ref))
    assert dev <= 2 * ref + 4, (dev, ref)


@pytest.mark.parametrize("m", [1, 2, 127, 128, 129, 257, 1030])
@pytest.mark.parametrize("per_problem", [False, True])
def test_columns_against_long_double(m, per_problem):
    """vp_basis (fp64) against the defining sums in long double with exp(-dt/tau) taken in long double: one row, one group,
    either side of a tile edge, the odd unaligned case, several tiles with a tail; shared and per-problem responses and
    grids.  Errors in the sensitivity units of the recurrence (irf_cases.column_errors); the limit is numpy's own sequential
    recurrence in the same dtype, in the same units, twice, plus 4 units for the different summation order of the scan.
    Measured on an MI355X: device 0.30 - 0.65 units, numpy 0.30 - 0.85."""
    _check_columns(m, np.float64, per_problem)


@pytest.mark.parametrize("m", [255, 256, 257, 602])
@pytest.mark.parametrize("per_problem", [False, True])
def test_columns_fp32_against_long_double(m, per_problem):
    """fp32: tiles of 256 rows, groups of four; the same rule at the rounded fp32 inputs"""
    _check_columns(m, np.float32, per_problem)


# ---- 3. the convention -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [129, 1030])
def test_an_impulse_response_gives_the_exponential_decay_column(m):
    """irf = [1, 0, 0, ...]: the column is exp(-(t - t_0)/tau) -- lag 0 included, no factor dt -- i.e. the VP_BASIS_EXP_DECAY
    column of a device-column handle on the grid t - t_0.  Both against the long-double value in units of eps (1 + i) |value|
    (l_i = i for an impulse): the scan kernel to the rule of the column test, the pointwise kernel to 2 units (its
    exponential's argument i dt / tau <= i / 2 carries half a rounding)."""
    B = 8
    t0, dt = 1.75, 0.02
    x = t0 + dt * np.arange(m)
    tau = (np.geomspace(2.0, 16000.0, B) * dt)[:, None]
    irf = np.zeros(m)
    irf[0] = 1.0
    dc = vp.BatchProblem(small_model(x, 1), np.zeros((B, m)), irf=irf)
    Phi, dPhi = dc.basis(tau)
    dc.close()
    pw = vp.BatchProblem(vp.multi_exponential_model(x - t0, [1.0], offset=False), np.zeros((B, m)), device_columns=True)
    Phi_e, dPhi_e = pw.basis(tau)
    pw.close()
    i = np.arange(m).astype(ic.L)
    dev = ref = pnt = 0.0
    for b in range(B):
        step = ic.grid_step(x)
        arg = i * ic.L(step) / ic.L(tau[b, 0])
        Fl = np.exp(-arg)
        Dl = Fl * i * ic.L(step) / ic.L(tau[b, 0]) ** 2
        F_n, _H, D_n = ic.recurrence(irf, step, tau[b, 0])
        dev = max(dev, ic.unit_errors(Phi[b, 0], Fl, i, EPS64), ic.unit_errors(dPhi[b, 0], Dl, i, EPS64))
        ref = max(ref, ic.unit_errors(F_n, Fl, i, EPS64), ic.unit_errors(D_n, Dl, i, EPS64))
        # (the pointwise kernel sees the rounded grid x - t_0: its own reference)
        tl = (x - t0).astype(ic.L)
        Fp = np.exp(-tl / ic.L(tau[b, 0]))
        pnt = max(pnt, ic.unit_errors(Phi_e[b, 0], Fp, i, EPS64), ic.unit_errors(dPhi_e[b, 0], Fp * tl / ic.L(tau[b, 0]) ** 2, i, EPS64))
        # the two references agree to the rounding of the grid itself
        assert np.abs(Fp - Fl).max() <= 1e-12
    print("impulse m=%d: scan %.3f, numpy recurrence %.3f, pointwise kernel %.3f [eps (1 + i) |value|]" % (m, dev, ref, pnt))
    assert dev <= 2 * ref + 4 and pnt <= 2
    assert np.abs(Phi - Phi_e).max() <= 1e-12


# ---- 4. - 6., 8. fits --------------------------------------------------------------------------------------------------
SEED = 20


@functools.lru_cache(maxsize=None)
def _fit_case(m, weighted, S):
    """data, oracle fits and the device fit of one case, shared by the tests below (nothing in it is modified)"""
    B = 48
    d = ic.lifetime_data(SEED + m + S, B, m, S=S)
    w = (0.5 + np.random.default_rng(3 + m).random(m)) if weighted else None
    cm = ic.lifetime_closures(d["x"], d["irf"])
    ref = oracle_fits(cm, d["Y"], d["guess"], w)
    return d, w, cm, ref


@pytest.mark.parametrize("m,weighted,S", [(200, False, 1), (200, True, 1), (1030, False, 1), (1030, True, 1), (200, False, 3)])
def test_fit_matches_the_oracle_and_the_stepped_fit_bit_for_bit(m, weighted, S):
    d, w, cm, ref = _fit_case(m, weighted, S)
    assert (ref[1] > 0).all()  # the oracle alone succeeds on every problem: none is excluded
    dc = vp.BatchProblem(ic.lifetime_model(d["x"]), d["Y"], weights=w, irf=d["irf"])
    a, C, rep = dc.fit(d["guess"])
    s = compare_with_oracle(rep, a, ref)
    print("lifetime fit m=%d weighted=%s S=%d: %s" % (m, weighted, S, s))
    # 8. the handle's state is the fitted point, columns included: statistics without a further call
    st = dc.statistics() if S == 1 else dc.global_statistics()
    assert (np.asarray(st["status"]) == 0).all()
    # 5. the stepped fit of an external handle, fed with vp_basis' columns: the same bits
    dc2 = vp.BatchProblem(ic.lifetime_model(d["x"]), d["Y"], weights=w, irf=d["irf"])
    ext = vp.BatchProblem(cm.shape(), d["Y"], weights=w)
    a2, C2, rep2, _steps = ext.fit_with_model(columns_from(dc2), d["guess"], check_every=3)
    assert np.array_equal(a, a2) and np.array_equal(C, C2) and report_equal(rep, rep2)
    if S == 1:  # ... and the statistics of the external handle at the fitted point, given the same cached state
        dc.set_params(a)
        st = dc.statistics()
        Phi_f, dPhi_f = dc2.basis(a)
        ext.set_params_with_basis(a, Phi_f, dPhi_f)
        se = ext.statistics()
        for key in ("cov", "reduced_chi2", "conf_sigma", "status"):
            assert np.array_equal(np.asarray(st[key]), np.asarray(se[key]), equal_nan=(key != "status")), key
    ext.close()
    dc2.close()
    dc.close()


def test_bounds():
    d, w, cm, ref = _fit_case(200, False, 1)
    B = d["Y"].shape[0]
    dc = vp.BatchProblem(ic.lifetime_model(d["x"]), d["Y"], irf=d["irf"])
    a0, C0, rep0 = dc.fit(d["guess"])
    dc.set_bounds([-np.inf, -np.inf], [np.inf, np.inf])
    a1, C1, rep1 = dc.fit(d["guess"])
    assert np.array_equal(a0, a1) and np.array_equal(C0, C1) and report_equal(rep0, rep1)
    lo, hi = np.array([0.2, 2.0]), np.array([2.0, 10.0])
    assert ((d["truth"] > lo) & (d["truth"] < hi) & (d["guess"] > lo) & (d["guess"] < hi)).all()
    dc.set_bounds(lo, hi)
    a2, _C2, rep2 = dc.fit(d["guess"])
    dc.close()
    assert ((a2 >= lo) & (a2 <= hi)).all()
    assert (rep2["termination"] > 0).all() and (rep0["termination"] > 0).all()
    rel = np.abs(rep2["objective"] - rep0["objective"]) / rep0["objective"]
    print("bounded lifetime fit: objective rel median %.2e max %.2e" % (np.median(rel), rel.max()))
    assert np.median(rel) <= K.EXTFIT["objective_rel_median_max"] and rel.max() <= K.EXTFIT["objective_rel_max_max"]


def test_device_tensors_and_fit_pipeline():
    """torch tensors in (the response included, copied on the device): the bits of the host-pointer handle; FitPipeline
    with irf= and a replaced response"""
    import torch
    d, w, cm, ref = _fit_case(200, False, 1)
    host = vp.BatchProblem(ic.lifetime_model(d["x"]), d["Y"], irf=d["irf"])
    a, C, rep = host.fit(d["guess"])
    irf2 = ic.response(200, centre=0.1, width=0.02)
    host.set_irf(irf2)
    b2, C2, rep2 = host.fit(d["guess"])
    host.close()
    assert not np.array_equal(a, b2)
    dev = torch.device("cuda:0")
    tt = lambda v: torch.as_tensor(v, device=dev)  # noqa: E731
    bp = vp.BatchProblem(ic.lifetime_model(d["x"]), tt(d["Y"]), irf=tt(d["irf"]))
    ad, Cd, repd = bp.fit(tt(d["guess"]))
    assert np.array_equal(ad.cpu().numpy(), a) and np.array_equal(Cd.cpu().numpy(), C) and report_equal(rep, repd)
    bp.close()
    pipe = vp.FitPipeline(ic.lifetime_model(d["x"]), tt(d["Y"]), n_slots=2, irf=tt(d["irf"]))
    o1 = pipe.submit(tt(d["Y"]), tt(d["guess"]))
    pipe.wait()
    pipe.set_irf(tt(irf2))
    o2 = [pipe.submit(tt(d["Y"]), tt(d["guess"])) for _ in range(2)]
    pipe.wait()
    torch.cuda.synchronize()
    assert np.array_equal(o1[0].cpu().numpy(), a) and report_equal(o1[2], rep)
    for o in o2:
        assert np.array_equal(o[0].cpu().numpy(), b2) and np.array_equal(o[1].cpu().numpy(), C2) and report_equal(o[2], rep2)
    pipe.close()


# ---- 7. search -----------------------------------------------------------------------------------------------------------
TAU1_GRID = (0.4, 0.6, 0.8, 1.0, 1.3, 1.6)
TAU2_GRID = (2.5, 3.2, 4.0, 4.8, 5.6, 6.5)


@pytest.mark.parametrize("irf_per_problem", [False, True])
def test_search(irf_per_problem):
    """a 6 x 6 grid of (tau1, tau2): numpy's argmin under the rule of tests/test_gpu_search.py (no problem is excluded: the
    two best numpy costs of every problem differ by more than 8 n m eps |y|^2) -- the shared route with a shared response,
    the candidate loop with one per problem"""
    B, m = 24, 200
    d = ic.lifetime_data(77, B, m, irf_per_problem=irf_per_problem)
    cand = vp.candidate_grid(TAU1_GRID, TAU2_GRID)
    cost_np, y2 = ic.lifetime_costs(d["irf"], d["dt"], cand, d["Y"])
    dc = vp.BatchProblem(ic.lifetime_model(d["x"]), d["Y"], irf=d["irf"])
    a, idx, cost = dc.search(cand)
    sc.check_fp64(idx, cost, cost_np, y2, 4, m, 1e-9, cap=0.0)
    assert np.array_equal(a, cand[idx])
    assert np.array_equal(np.asarray(dc.params()), a) and np.array_equal(np.asarray(dc.cost()), cost)
    if not irf_per_problem:  # the same data through the candidate loop (a per-problem copy of the response): the same indices
        dc.set_irf(np.broadcast_to(d["irf"], (B, m)).copy())
        _a2, idx2, _cost2 = dc.search(cand)
        assert np.array_equal(idx2, idx)
    dc.close()


# ---- 8. state and refusals ---------------------------------------------------------------------------------------------
def test_state_and_refusals():
    d, w, cm, ref = _fit_case(200, False, 1)
    B, m = d["Y"].shape
    g = d["guess"]
    dc = vp.BatchProblem(ic.lifetime_model(d["x"]), d["Y"])
    cand = vp.candidate_grid(TAU1_GRID, TAU2_GRID)
    calls = [lambda: dc.set_params(g), lambda: dc.evaluate(g), lambda: dc.basis(g), lambda: dc.fit(g), lambda: dc.search(cand),
             lambda: dc.statistics(), lambda: dc.global_statistics()]
    for i, call in enumerate(calls):
        with pytest.raises(vp.VarproHipError) as e:
            call()
        assert e.value.code == -1, i  # VP_ERR_INVALID
        if i < 5:
            assert "vp_set_irf" in str(e.value), str(e.value)
    dc.set_irf(d["irf"])
    ev = dc.evaluate(g)
    assert (np.asarray(ev["status"]) == 0).all()
    # a replaced response changes the next evaluation, and invalidates the cached one
    dc.set_irf(ic.response(m, centre=0.1, width=0.02))
    with pytest.raises(vp.VarproHipError):
        dc.cost()
    ev2 = dc.evaluate(g)
    assert not np.array_equal(np.asarray(ev2["cost"]), np.asarray(ev["cost"]))
    dc.set_irf(d["irf"])
    assert np.array_equal(np.asarray(dc.evaluate(g)["cost"]), np.asarray(ev["cost"]))
    # tau = 0 (and a negative and a NaN tau) latch their problems alone
    bad = g.copy()
    bad[5, 0] = 0.0
    bad[9, 1] = -1.0
    bad[17, 0] = np.nan
    idx = [5, 9, 17]
    good = np.setdiff1d(np.arange(B), idx)
    evb = dc.evaluate(bad)
    stt = np.asarray(evb["status"])
    assert (stt[idx] != 0).all() and (stt[good] == 0).all()
    assert np.array_equal(np.asarray(evb["cost"])[good], np.asarray(ev["cost"])[good])
    a, C, rep = dc.fit(bad)
    assert (rep["termination"][idx] < 0).all()
    dc.close()
    dc = vp.BatchProblem(ic.lifetime_model(d["x"]), d["Y"][good], irf=d["irf"])
    a2, C2, rep2 = dc.fit(g[good])
    dc.close()
    assert np.array_equal(a[good], a2) and np.array_equal(C[good], C2) and report_equal(rep[good], rep2)
    # vp_set_irf on a handle without these kinds, and a non-uniform host grid at the C boundary
    import ctypes as C_
    bp = vp.BatchProblem(vp.multi_exponential_model(d["x"], [1.0, 4.0]), d["Y"], device_columns=True)
    assert bp.lib.vp_set_irf(bp._h, C_.c_void_p(d["irf"].ctypes.data), 0) == -1
    bp.close()
    mdl = ic.lifetime_model(d["x"])
    xb = d["x"].copy()
    xb[7] += 2e-6 * d["dt"]
    h = C_.c_void_p()
    desc = mdl.desc()
    rc = bp.lib.vp_batch_create(C_.byref(h), C_.byref(desc), 0, m, 1, B, C_.c_void_p(xb.ctypes.data),
                                C_.c_void_p(d["Y"].ctypes.data), None, -1.0, 0, 0, None)
    assert rc == -1 and not h.value
    # the single-problem surface
    prob = (vp.SeparableProblemBuilder.new(ic.lifetime_model(d["x"])).observations(d["Y"][0])
            .instrument_response(d["irf"]).build())
    prob.set_params(g[0])
    assert np.allclose(prob.residuals(), np.asarray(ev["r"])[0], rtol=0, atol=1e-12 * np.abs(d["Y"][0]).max())
    prob.close()
