"""GPU tier of fixed nonlinear parameters (vp_batch_create_fixed / vp_set_fixed_values; BatchProblem(fixed=...)).  The
handle is the reduced model and only the column kernels' fixed siblings (varpro_amd/csrc/vp_cols.hpp, vp_irf.hpp) know the full
parameter vector, so the tests are: the siblings' columns against the plain kernels' BIT FOR BIT (the same basis_at
statements), an all-zero mask against a plain handle bit for bit, fits against the CPU oracle driven by the reduced closures
(tests/fixed_cases.py) under the unchanged K.EXTFIT contract, the caller-evaluated route fed with the handle's own columns
bit for bit, and the composition with bounds, statistics, search, Poisson re-weighting and replaced values.  The CPU tier
(tests/test_fixed_host.py) asserts what the contract presupposes: the oracle succeeds on 48 of 48 problems of every case."""
import ctypes as C

import numpy as np
import pytest

import contracts as K
import fixed_cases as fc
import irf_cases as ic
import poisson_cases as poc
import varpro_amd as vp
from varpro_amd import _lib
from test_gpu_bounds import inside, transformed_oracle_fits
from test_gpu_external import oracle_problem
from test_gpu_extfit import compare_with_oracle
from test_gpu_peak_kinds import report_equal

pytestmark = pytest.mark.gpu
INF = np.inf


def _problem(case, Y, values, dtype=np.float64, x=None, **extra):
    """the handle with the case's parameters held at ``values`` ((q,) or (B, q) in full order)"""
    kw = dict(case.kwargs)
    kw.update(extra)
    mdl = case.model(dtype)
    return vp.BatchProblem(mdl, np.asarray(Y, dtype=dtype), x=x, fixed=case.fixed_dict(values), **kw)


def _plain(case, Y, dtype=np.float64, x=None, **extra):
    kw = dict(case.kwargs)
    kw.update(extra)
    return vp.BatchProblem(case.model(dtype), np.asarray(Y, dtype=dtype), x=x, device_columns=True, **kw)


# ---- 1. columns, bit for bit ------------------------------------------------------------------------------------------------
# fp64 m: a single row, one group, both sides of a scan tile (128 rows), odd lengths (element-wise stores); fp32: 256 rows
@pytest.mark.parametrize("dtype,ms", [(np.float64, (1, 2, 127, 128, 129)), (np.float32, (255, 256, 257))])
@pytest.mark.parametrize("key", fc.CASE_KEYS)
def test_columns_equal_the_plain_kernels_bit_for_bit(key, dtype, ms):
    B = 5
    for m in ms:
        if key == "c" and m == 1:
            continue  # (the periodic kind needs m >= 2: creation refuses a single sample)
        case, x, alpha = fc.columns_case(key, m, B=B)
        alpha = alpha.astype(dtype)
        for per_problem in (False, True):
            values = alpha.astype(np.float64) if per_problem else alpha[0].astype(np.float64)
            at = alpha.copy()                                    # the expanded point: fixed entries as the kernel reads them
            at[:, case.held] = np.asarray(values, dtype=dtype)[..., case.held]
            fx = _problem(case, np.zeros((B, m)), values, dtype)
            pl = _plain(case, np.zeros((B, m)), dtype)
            junk = np.where(np.isin(np.arange(alpha.shape[1]), case.held), dtype(-7.0), alpha)  # fixed columns are ignored
            Phi, dPhi = fx.basis(junk)
            Phi0, dPhi0 = pl.basis(at)
            assert dPhi.shape == (B, len(case.free_pairs), m)
            assert np.array_equal(Phi, Phi0, equal_nan=True), (key, m, per_problem)
            assert np.array_equal(dPhi, dPhi0[:, case.free_pairs], equal_nan=True), (key, m, per_problem)
            assert np.isfinite(Phi).all() and np.isfinite(dPhi).all()
            fx.close()
            pl.close()


def test_columns_on_per_problem_grids_and_without_invariant_columns():
    B, m = 5, 129
    case, x, alpha = fc.columns_case("a", m, B=B)
    xs = x[None, :] + np.linspace(0.0, 0.4, B)[:, None]
    at = alpha.copy()
    fx = _problem(case, np.zeros((B, m)), alpha, x=xs)
    pl = _plain(case, np.zeros((B, m)), x=xs)
    for skip in (False, True):
        Phi, dPhi = fx.basis(alpha, skip_invariant=skip)
        Phi0, dPhi0 = pl.basis(at, skip_invariant=skip)
        assert Phi.shape == (B, 3 if skip else 4, m)
        assert np.array_equal(Phi, Phi0) and np.array_equal(dPhi, dPhi0[:, case.free_pairs])
    fx.close()
    pl.close()
    # the trap case without its constant column: the column numbering of Phi moves, the free pairs do not
    case, x, alpha = fc.columns_case("d", m, B=B)
    fx = _problem(case, np.zeros((B, m)), alpha[0])
    pl = _plain(case, np.zeros((B, m)))
    at = alpha.copy()
    at[:, case.held] = alpha[0, case.held]
    Phi, dPhi = fx.basis(alpha, skip_invariant=True)
    Phi0, dPhi0 = pl.basis(at, skip_invariant=True)
    assert Phi.shape == (B, 5, m) and np.array_equal(Phi, Phi0) and np.array_equal(dPhi, dPhi0[:, case.free_pairs])
    fx.close()
    pl.close()


# ---- 2. an all-zero mask is an ordinary device-column handle -------------------------------------------------------------
def test_all_zero_mask_is_a_plain_device_column_handle():
    case, x, Y, guess, _values, _w = fc.fit_case("a")
    pl = _plain(case, Y)
    a0, C0, rep0 = pl.fit(guess)
    r0, st0 = np.asarray(pl.residuals()), pl.statistics()
    pl.close()
    bp = vp.BatchProblem(case.model(), Y, fixed={})
    assert type(bp).__name__ == "FixedBatchProblem" and bp.q == 4 and bp.p == 4
    a1, C1, rep1 = bp.fit(guess)
    assert np.array_equal(a0, a1) and np.array_equal(C0, C1) and report_equal(rep0, rep1)
    assert np.array_equal(r0, np.asarray(bp.residuals()))
    st1 = bp.statistics()
    for key in ("cov", "reduced_chi2", "conf_sigma", "status"):
        assert np.array_equal(np.asarray(st0[key]), np.asarray(st1[key]), equal_nan=(key != "status")), key
    assert np.array_equal(np.asarray(bp.params()), a1)
    bp.close()


# ---- 3. fits against the oracle of the reduced model -------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("key", fc.FIT_KEYS)
def test_fit_matches_the_oracle_of_the_reduced_model(key, weighted):
    case, _x, Y, guess, values, w = fc.fit_case(key, weighted)
    ref = fc.fit_reference(key, weighted)
    assert (ref[1] > 0).all()
    bp = _problem(case, Y, values, weights=w)
    a, Cc, rep = bp.fit(guess)
    assert a.shape == guess.shape and np.array_equal(a[:, case.held], values[:, case.held])  # full order, fixed entries filled in
    s = compare_with_oracle(rep, a[:, case.free], ref)
    print("fixed fit %s weighted=%s: %s" % (key, weighted, s))
    assert np.array_equal(np.asarray(bp.params()), a) and np.array_equal(np.asarray(bp.linear_coefficients()), Cc)
    r = np.asarray(bp.residuals())
    assert (np.abs(0.5 * (r ** 2).sum(1) - rep["objective"]) <= 1e-9 * rep["objective"]).all()
    for b in range(0, fc.B_FIT, 7):  # coefficients of the fitted point
        p = oracle_problem(case.reduced(values[b]), Y[b], w=w)
        p.set_params(a[b, case.free])
        assert np.abs(Cc[b] - p.linear_coefficients()).max() <= 1e-9 * np.abs(Cc[b]).max()
    bp.close()


def test_per_problem_values_are_indexed_by_problem_not_by_list_slot():
    """neighbouring problems are held at tau2 ~ 3 and ~ 6: once the active set has compacted, a value taken by the list slot
    belongs to another problem, and the fit of that problem lands on another objective"""
    case, _x, Y, guess, values = fc.alternating_lifetime_case()
    ref = fc.reduced_oracle_fits(case, Y, guess, values)
    assert (ref[1] > 0).all() and np.ptp(ref[2]) >= 2, "every fit ends at the same step: the active set would never compact"
    assert (np.abs(np.diff(values[:, 1])) > 2.5).all()
    bp = _problem(case, Y, values)
    a, _C, rep = bp.fit(guess)
    bp.close()
    s = compare_with_oracle(rep, a[:, case.free], ref)
    print("alternating fixed tau2: %s" % s)


def test_global_fit_of_three_right_hand_sides():
    """case (b), S = 3, under the contracts of tests/test_gpu_bounds.py::test_global_fit_of_three_right_hand_sides"""
    S, B, m = 3, 8, 200
    d = ic.lifetime_data(20 + m + S, B, m, S=S)
    x = d["x"]
    case = fc.Case("b", lambda dt=np.float64: ic.lifetime_model(x.astype(dt), dt), ic.lifetime_closures(x, d["irf"]), fc.EXP_NAMES,
                   ("tau2",), dict(irf=d["irf"]))
    values = np.zeros((B, 2))
    values[:, 1] = d["truth"][:, 1]
    bp = _problem(case, d["Y"], values)
    a1, C1, rep = bp.fit(d["guess"])
    assert np.asarray(C1).shape == (B, S, 4)
    n_ok = 0
    for b in range(B):
        p = oracle_problem(case.reduced(values[b]), d["Y"][b])
        p.set_params(d["guess"][b, case.free])
        r = p.fit()
        assert (rep["termination"][b] > 0) == (r.termination > 0), (b, rep[b], r.termination)
        if r.termination > 0:
            n_ok += 1
            assert abs(rep["objective"][b] - r.objective) <= 1e-6 * r.objective, (b, rep["objective"][b], r.objective)
            assert abs(int(rep["n_evals"][b]) - int(r.n_evals)) <= 4
            a_ref = np.asarray(p.params())
            assert np.abs(a1[b, case.free] - a_ref).max() <= 1e-5 * np.abs(a_ref).max()
            Cr = np.asarray(p.linear_coefficients()).reshape(S, 4)
            assert np.abs(C1[b] - Cr).max() <= 1e-5 * np.abs(Cr).max()
    assert n_ok >= 0.95 * B
    g = bp.global_statistics(want_confidence_sigma=True)
    assert (np.asarray(g["status"]) == 0).all() and g["free"].tolist() == [0]
    for key in ("cov_alpha", "reduced_chi2", "coef_cov", "coef_alpha_cov", "conf_sigma"):
        assert np.isfinite(np.asarray(g[key])).all(), key
    cov = np.asarray(g["cov_alpha"])
    assert cov.shape == (B, 2, 2) and (cov[:, 0, 0] > 0).all() and not cov[:, 1, :].any() and not cov[:, :, 1].any()
    assert np.asarray(g["coef_alpha_cov"]).shape == (B, S, 4, 2) and not np.asarray(g["coef_alpha_cov"])[..., 1].any()
    assert g["dof"] == m * S - 4 * S - 1
    bp.close()


# ---- 4. the caller-evaluated route on the handle's own columns: the same bits ---------------------------------------------
def test_caller_evaluated_fit_on_the_reduced_shape_is_bit_identical():
    B, m = 24, 200
    d = fc.trap_data(9, B, m)
    x = d["x"]
    case = fc.Case("d", lambda dt=np.float64: fc.trap_model(x.astype(dt), dt), d["cm"], fc.TRAP_NAMES, fc.TRAP_FIXED, dict(irf=d["irf"]))
    values = np.zeros_like(d["truth"])
    values[:, case.held] = d["truth"][:, case.held]
    dc = _problem(case, d["Y"], values)
    a, Cc, rep = dc.fit(d["guess"])
    assert (vp.BatchProblem.report_to_numpy(rep)["termination"] > 0).mean() >= 0.9
    dc2 = _problem(case, d["Y"], values)
    red = case.reduced(values[0])
    ext = vp.BatchProblem(red.shape(), d["Y"])
    full = d["guess"].copy()

    def evaluate(alpha_free, want):
        full[:, case.free] = np.asarray(alpha_free)
        return dc2.basis(full)
    a2, C2, rep2, _steps = ext.fit_with_model(evaluate, d["guess"][:, case.free], check_every=3)
    assert np.array_equal(a[:, case.free], a2) and np.array_equal(Cc, C2) and report_equal(rep, rep2)
    ext.close()
    dc2.close()
    dc.close()


# ---- 5. bounds compose ---------------------------------------------------------------------------------------------------
def test_infinite_bounds_change_nothing_and_an_active_box_matches_the_transformed_oracle():
    case, _x, Y, guess, _values, _w = fc.fit_case("a")
    values = np.array([0.0, 0.65, 0.0, 0.85])  # both widths at one value for the batch
    bp = _problem(case, Y, values)
    a0, C0, rep0 = bp.fit(guess)
    bp.set_bounds(np.full(4, -INF), np.full(4, INF))
    a1, C1, rep1 = bp.fit(guess)
    assert np.array_equal(a0, a1) and np.array_equal(C0, C1) and report_equal(rep0, rep1)
    # a box on the free centres that cuts optima off (the widths' entries of the full-order box are ignored)
    lo, hi = np.array([2.8, -INF, 6.3, -INF]), np.array([3.2, INF, 6.7, INF])
    outside = ~((a0[:, case.free] >= lo[case.free]) & (a0[:, case.free] <= hi[case.free])).all(1) & (rep0["termination"] > 0)
    assert outside.sum() >= 1, "the box cuts nothing off: the test would pass vacuously"
    g = guess.copy()
    g[:, case.free] = inside(guess[:, case.free], lo[case.free], hi[case.free])
    ref = transformed_oracle_fits(case.reduced(values), Y, g[:, case.free], lo[case.free], hi[case.free])
    bp.set_bounds(lo, hi)
    a, _C, rep = bp.fit(g)
    bp.close()
    assert (a[:, case.free] >= lo[case.free]).all() and (a[:, case.free] <= hi[case.free]).all()  # bounds included, no tolerance
    assert np.array_equal(a[:, case.held], np.tile(values[case.held], (fc.B_FIT, 1)))
    _a_ref, term, nev, obj = ref
    ok = term > 0
    assert ((rep["termination"] > 0) == ok).all()
    assert (rep["termination"] == term).all(), "termination reasons differ on %s" % np.nonzero(rep["termination"] != term)[0][:8]
    rel = np.abs(rep["objective"] - obj)[ok] / obj[ok]
    share = float((np.abs(rep["n_evals"] - nev) <= 3).mean())
    print("active box on fixed-width peaks: %d of %d optima outside; objective rel median %.3e max %.3e; evaluations within 3 "
          "on %.4f" % (outside.sum(), len(outside), np.median(rel), rel.max(), share))
    assert np.median(rel) <= K.EXTFIT["objective_rel_median_max"] and rel.max() <= K.EXTFIT["objective_rel_max_max"]
    # fits that converge ONTO a bound end on xtol with cos u -> 0, where the evaluation count is sensitive to rounding: the
    # rule of tests/test_gpu_bounds.py::test_active_box_keeps_every_parameter_inside -- the measured share minus 0.05 (two
    # problems of 48), never below 0.8
    MEASURED_SHARE = 0.9792  # 47 of 48, first run on an MI355X
    assert share >= max(0.8, MEASURED_SHARE - 0.05), share


# ---- 6. statistics of the problem that was solved -----------------------------------------------------------------------
def test_statistics_are_those_of_the_reduced_model():
    case, _x, Y, guess, values, _w = fc.fit_case("a")
    n, q = 4, 4
    bp = _problem(case, Y, values)
    a, _C, rep = bp.fit(guess)
    st = bp.statistics()
    cov = np.asarray(st["cov"])
    assert cov.shape == (fc.B_FIT, n + q, n + q) and st["free"].tolist() == case.free and st["dof"] == fc.M_FIT - n - len(case.free)
    assert (np.asarray(st["status"]) == 0).all() and np.asarray(st["conf_sigma"]).shape == (fc.B_FIT, fc.M_FIT)
    for k in case.held:  # rows and columns of fixed parameters: exactly 0
        assert not cov[:, n + k, :].any() and not cov[:, :, n + k].any()
    keep = np.concatenate([np.arange(n), n + np.array(case.free)])
    pl = _plain(case, Y)
    pl.set_params(a)
    cov_plain = np.asarray(pl.statistics()["cov"])
    pl.close()
    for b in range(0, fc.B_FIT, 6):
        p = oracle_problem(case.reduced(values[b]), Y[b])
        p.set_params(a[b, case.free])
        so = p.statistics()
        block = cov[b][keep[:, None], keep[None, :]]
        assert abs(st["reduced_chi2"][b] - so["reduced_chi2"]) <= 1e-9 * so["reduced_chi2"]
        assert np.abs(block - so["cov"]).max() <= 1e-7 * np.abs(so["cov"]).max()
        # ... and NOT the block of the unconstrained linearisation: the test can tell the two apart
        assert np.abs(block - cov_plain[b][keep[:, None], keep[None, :]]).max() > 1e-7 * np.abs(so["cov"]).max()
    bp.close()


# ---- 7. replacing the values -----------------------------------------------------------------------------------------------
def test_three_replaced_values_equal_three_fresh_handles():
    case, _x, Y, guess, _values, _w = fc.fit_case("b")
    bp = _problem(case, Y, np.array([0.0, 3.5]))
    per = np.linspace(3.0, 6.0, fc.B_FIT)
    for tau2 in (3.5, 4.5, per):
        if not (np.ndim(tau2) == 0 and tau2 == 3.5):
            bp.set_fixed(tau2=tau2)
        a, Cc, rep = bp.fit(guess)
        fresh = vp.BatchProblem(case.model(), Y, fixed={"tau2": tau2}, **case.kwargs)
        a0, C0, rep0 = fresh.fit(guess)
        fresh.close()
        assert np.array_equal(a, a0) and np.array_equal(Cc, C0) and report_equal(rep, rep0)
        assert np.array_equal(a[:, 1], np.broadcast_to(tau2, (fc.B_FIT,)))
    bp.close()


# ---- 8. composition -----------------------------------------------------------------------------------------------------
def test_search_ranks_as_the_costs_evaluated_one_by_one():
    case, _x, Y, _guess, values, _w = fc.fit_case("e")
    cand = np.stack([np.full(9, -1.0), np.linspace(2.0, 7.0, 9)], 1)  # (K, q) in full order; the column of tau1 is ignored
    for v in (np.array([1.0, 0.0]), values):                         # shared values: the shared route; per problem: the loop
        bp = _problem(case, Y, v)
        a, idx, cost = bp.search(cand)
        costs = np.empty((fc.B_FIT, len(cand)))
        for k in range(len(cand)):
            bp.set_params(cand[k])
            costs[:, k] = np.asarray(bp.cost())
        assert np.array_equal(np.asarray(idx), costs.argmin(1))
        assert np.array_equal(a[:, 1], cand[np.asarray(idx), 1]) and np.array_equal(a[:, 0], np.broadcast_to(v[..., 0], (fc.B_FIT,)))
        assert np.array_equal(np.asarray(cost), costs.min(1))
        a2, _C2, rep2 = bp.fit_from_search(cand)
        assert a2.shape == (fc.B_FIT, 2) and np.array_equal(a2[:, 0], a[:, 0])
        bp.close()


def test_poisson_fit_with_a_fixed_lifetime():
    """one re-weighted round against the oracle of the reduced model at the mirror's weights of the device's best fit (the
    contract of tests/test_gpu_poisson.py::test_one_round_against_the_oracle), then fit_poisson end to end"""
    wl = poc.lifetime(poc.LIFETIME_SEED, poc.B_FIT)
    cm = ic.lifetime_closures(wl.x, wl.irf)
    case = fc.Case("b", lambda dt=np.float64: wl.model(dt), cm, fc.EXP_NAMES, ("tau2",), dict(irf=wl.irf))
    values = np.zeros_like(wl.truth)
    values[:, 1] = wl.truth[:, 1]
    bp = _problem(case, wl.Y, values, weights="neyman")
    a1, _C1, rep1 = bp.fit(wl.guess)
    assert (rep1["termination"] > 0).all()
    F = np.asarray(bp.best_fit())
    bp.poisson_reweight(wl.Y, "model")
    a2, _C2, rep2 = bp.fit(a1)
    W, _ = poc.reweight_mirror(wl.Y, F)
    parts = []
    for b in range(poc.B_FIT):
        p = oracle_problem(case.reduced(values[b]), wl.Y[b], w=W[b])
        p.set_params(a1[b, case.free])
        r = p.fit()
        parts.append((np.asarray(p.params()), r.termination, r.n_evals, r.objective))
    ref = (np.stack([p[0] for p in parts]), np.array([p[1] for p in parts], dtype=np.int32),
           np.array([p[2] for p in parts], dtype=np.int32), np.array([p[3] for p in parts]))
    assert (ref[1] > 0).all()
    s = compare_with_oracle(rep2, a2[:, case.free], ref)
    print("fixed tau2, one re-weighted round: %s" % s)
    a, Cc, rep, info = bp.fit_poisson(wl.Y, wl.guess)
    assert (rep["termination"] > 0).all() and np.array_equal(a[:, 1], values[:, 1]) and a.shape == (poc.B_FIT, 2)
    D = np.asarray(info["deviance"])
    assert np.isfinite(D).all() and (D > 0).all()
    assert np.allclose(np.asarray(info["reduced_deviance"]), D / (wl.Y.shape[1] - 4 - 1), rtol=1e-15)  # dof counts the free parameter
    assert np.array_equal(np.asarray(bp.params()), a)
    bp.close()


def test_device_tensors_and_the_pipeline():
    import torch
    case, _x, Y, guess, values, _w = fc.fit_case("b")
    host = _problem(case, Y, values)
    a, Cc, rep = host.fit(guess)
    host.close()
    dev = torch.device("cuda:0")
    fixed_dev = {"tau2": torch.as_tensor(values[:, 1].copy(), device=dev)}
    kw = dict(irf=torch.as_tensor(case.kwargs["irf"], device=dev))
    bp = vp.BatchProblem(case.model(), torch.as_tensor(Y, device=dev), fixed=fixed_dev, **kw)
    ad, Cd, repd = bp.fit(torch.as_tensor(guess, device=dev))
    assert np.array_equal(ad.cpu().numpy(), a) and np.array_equal(Cd.cpu().numpy(), Cc) and report_equal(rep, repd)
    assert np.array_equal(bp.params().cpu().numpy(), a)
    bp.close()
    with vp.FitPipeline(case.model(), torch.as_tensor(Y, device=dev), fixed=fixed_dev, **kw) as pipe:
        ap, Cp, repp, slot = pipe.submit(torch.as_tensor(Y, device=dev), torch.as_tensor(guess, device=dev))
        pipe.wait(slot)
        assert np.array_equal(ap.cpu().numpy(), a) and np.array_equal(Cp.cpu().numpy(), Cc) and report_equal(rep, repp)
        pipe.set_fixed(tau2=fixed_dev["tau2"])  # (the same values again, on every slot)
        ap, Cp, repp, slot = pipe.submit(torch.as_tensor(Y, device=dev), torch.as_tensor(guess, device=dev))
        pipe.wait(slot)
        assert np.array_equal(ap.cpu().numpy(), a) and report_equal(rep, repp)
    with vp.FitPipeline(case.model(), torch.as_tensor(Y, device=dev), **kw) as pipe:
        with pytest.raises(ValueError):
            pipe.set_fixed(tau2=3.0)


# ---- 9. refusals and persistence ---------------------------------------------------------------------------------------
def test_refusals():
    lib = vp.load_library()
    m, B = 64, 2
    x = np.linspace(0.0, 10.0, m)
    Y = np.ones((B, m))
    desc = fc.peaks_model(x).desc()
    vals = (C.c_double * 4)(3.0, 0.7, 6.4, 0.9)

    def create(d, mask, values, flags=_lib.VP_FLAG_OWN_STREAM):
        h = C.c_void_p()
        cm = None if mask is None else (C.c_int32 * 4)(*mask)
        rc = lib.vp_batch_create_fixed(C.byref(h), C.byref(d), _lib.VP_F64, m, 1, B, C.c_void_p(x.ctypes.data), C.c_void_p(Y.ctypes.data),
                                       None, -1.0, flags, 0, None, cm, None if values is None else C.cast(values, C.c_void_p), 0)
        if h.value:
            lib.vp_batch_destroy(h)
        return rc
    assert create(desc, [0, 1, 0, 1], vals) == _lib.VP_ERR_OK
    assert create(desc, None, vals) == _lib.VP_ERR_INVALID              # a null mask
    assert create(desc, [0, 2, 0, 0], vals) == _lib.VP_ERR_INVALID      # a mask entry other than 0 or 1
    assert create(desc, [0, -1, 0, 0], vals) == _lib.VP_ERR_INVALID
    assert create(desc, [1, 1, 1, 1], vals) == _lib.VP_ERR_INVALID      # no free parameter left
    assert create(desc, [0, 1, 0, 0], None) == _lib.VP_ERR_INVALID      # null values with a fixed parameter
    assert create(desc, [0, 0, 0, 0], None) == _lib.VP_ERR_OK           # ... which an all-zero mask does not need
    ext = fc.peaks_model(x).desc()
    ext.kind[0] = _lib.VP_BASIS_EXTERNAL
    assert create(ext, [0, 1, 0, 0], vals) == _lib.VP_ERR_UNSUPPORTED   # a caller-evaluated descriptor
    # vp_set_fixed_values: only on a handle created fixed, not with null values, not during a stepped fit
    plain = vp.BatchProblem(fc.peaks_model(x), Y)
    assert lib.vp_set_fixed_values(plain._h, C.cast(vals, C.c_void_p), 0) == _lib.VP_ERR_UNSUPPORTED
    plain.close()
    bp = vp.BatchProblem(fc.peaks_model(x), Y, fixed={"s1": 0.7})
    assert lib.vp_set_fixed_values(bp._h, None, 0) == _lib.VP_ERR_INVALID
    assert lib.vp_set_fixed_values(bp._h, C.cast(vals, C.c_void_p), 0) == _lib.VP_ERR_OK
    with pytest.raises(ValueError):
        bp.set_fixed(mu1=1.0)
    with pytest.raises(ValueError):
        vp.BatchProblem(fc.peaks_model(x), Y, fixed={"sigma": 1.0})
    # a descriptor without nonlinear parameters and its empty mask: what vp_batch_create answers for that descriptor, not
    # "no free parameter left"
    line = fc.peaks_model(x).desc()
    line.n_basis, line.n_params = 2, 0
    line.kind[0], line.kind[1] = vp.basis.LINEAR, vp.basis.CONST
    for j in range(2):
        line.param[j][0] = line.param[j][1] = -1
    h0 = C.c_void_p()
    rc0 = lib.vp_batch_create(C.byref(h0), C.byref(line), _lib.VP_F64, m, 1, B, C.c_void_p(x.ctypes.data), C.c_void_p(Y.ctypes.data),
                              None, -1.0, _lib.VP_FLAG_OWN_STREAM, 0, None)
    if h0.value:
        lib.vp_batch_destroy(h0)
    assert create(line, [0, 0, 0, 0], None) == rc0
    with pytest.raises(ValueError):  # lower == upper on a free parameter stays refused: fixing is done at creation
        bp.set_bounds([3.0, 0.0, 6.0, 0.1], [3.0, 0.0, 7.0, 2.0])
    bp.close()


def test_a_bad_value_latches_its_problem_alone_and_the_handle_survives_new_observations():
    case, _x, Y, guess, values, _w = fc.fit_case("b")
    good = _problem(case, Y, values)
    a0, C0, rep0 = good.fit(guess)
    bad_values = values.copy()
    bad_values[3, 1], bad_values[5, 1] = np.nan, 0.0
    bp = _problem(case, Y, bad_values)
    a, Cc, rep = bp.fit(guess)
    others = np.ones(fc.B_FIT, dtype=bool)
    others[[3, 5]] = False
    assert (rep["termination"][[3, 5]] <= 0).all() and (rep["termination"][others] > 0).all()
    assert np.array_equal(a[others], a0[others]) and np.array_equal(Cc[others], C0[others])
    assert np.array_equal(rep["objective"][others], rep0["objective"][others]) and np.array_equal(rep["n_evals"][others], rep0["n_evals"][others])
    st = np.asarray(bp.status())
    assert (st[[3, 5]] != 0).all() and (st[others] == 0).all()
    bp.close()
    # the mask and the values stay with the handle across set_observations
    Y2 = Y[::-1].copy()
    good.set_observations(Y2)
    a1, C1, rep1 = good.fit(guess)
    fresh = _problem(case, Y2, values)
    a2, C2, rep2 = fresh.fit(guess)
    assert np.array_equal(a1, a2) and np.array_equal(C1, C2) and report_equal(rep1, rep2)
    fresh.close()
    good.close()
