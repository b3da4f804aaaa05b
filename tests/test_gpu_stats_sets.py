"""vp_statistics and vp_best_fit of EVERY compiled kernel set against the oracle (tests/stats_cases.py holds the table, the
references and the tolerances; tests/test_stats_cases_host.py checks the table against the registry on the CPU).

Every case first asserts, through vp_debug_kernel_set, that its handle runs on the set the case names.  Parameters are set
with set_params (no fit), so a case is deterministic and cannot lose problems; the fits have their own test at the end."""
import numpy as np
import pytest

import stats_cases as SC
import varpro_amd as vp

pytestmark = pytest.mark.gpu
KEYS = ("chi2", "cov", "sigma", "cov_unit", "sigma_unit", "best_fit")
ids = lambda cases: [SC.case_id(c) for c in cases]  # noqa: E731


def make_handle(c, rows=None, **overrides):
    """the handle of a case (rows: a subset of its problems); asserts the kernel set it landed on"""
    d = dict(SC.case_data(c), **overrides)
    pick = (lambda a: a) if rows is None else (lambda a: np.ascontiguousarray(a[rows]))
    x = d["x"] if d["x"].ndim == 1 else pick(d["x"])
    w = d["w"] if d["w"] is None or d["w"].ndim == 1 else pick(d["w"])
    bp = vp.BatchProblem(d["model"], pick(d["Y"]), x=x, weights=w, stream_rows=c.stream)
    got = bp.kernel_set()
    assert got == c.set, "%s runs on %s" % (SC.case_id(c), SC.set_name(got))
    return bp


def compare(c, b, st, bf, ref, y, label=""):
    """problem b of a device result against one record of stats_cases.reference_at: prints every figure, then asserts"""
    assert ref["stats"] is not None
    assert st["status"][b] == 0 and st["dof"] == ref["stats"]["dof"]
    e, tol = SC.device_errors(st, bf, b, ref, y), ref["tol"]
    print("%s%s problem %d: kappa_s %.2e  " % (SC.case_id(c), label, b, ref["kappa_s"])
          + "  ".join("%s %.2e / %.2e" % (k, e[k], tol[k]) for k in KEYS))
    for k in KEYS:
        assert e[k] <= tol[k], (SC.case_id(c), b, k, e[k], tol[k])
    return e


def run(c):
    d = SC.case_data(c)
    with make_handle(c) as bp:
        bp.set_params(d["alpha"])
        return bp.statistics(), bp.best_fit(), bp.residuals()


@pytest.mark.parametrize("c", SC.CASES + SC.PER_PROBLEM_CASES, ids=ids(SC.CASES + SC.PER_PROBLEM_CASES))
def test_statistics_and_best_fit_of_every_kernel_set(c):
    d, refs = SC.case_data(c), SC.reference(c)
    st, bf, r = run(c)
    assert st["cov"].shape == (SC.B, refs[0]["stats"]["cov"].shape[0], refs[0]["stats"]["cov"].shape[0])
    for b in range(SC.B):
        _x, y, w = SC.problem_inputs(d, b)
        compare(c, b, st, bf, refs[b], y)
        assert np.array_equal(st["cov"][b], st["cov"][b].T)
        # the device's own residuals are w (y - best fit), to the bound of the best fit
        rw = (y - bf[b].astype(np.float64)) * (1.0 if w is None else w)
        assert np.abs(rw - r[b]).max() <= refs[b]["tol"]["best_fit"] * np.abs(y).max(), b
        assert np.abs(r[b] - refs[b]["residuals"]).max() <= 2 * refs[b]["tol"]["best_fit"] * np.abs(y).max(), b


@pytest.mark.parametrize("shape,dtype,kset", SC.DOF_EDGE_SETS, ids=[s[0] + "@" + SC.set_name(s[2]) for s in SC.DOF_EDGE_SETS])
def test_degrees_of_freedom_edge(shape, dtype, kset):
    # dof = 1 is computed, dof = 0 and dof = -1 are reported (FitStatisticsError::Underdetermined) and leave NaN
    c = SC.dof_edge_case(shape, dtype, kset, 1)
    d, refs = SC.case_data(c), SC.reference(c)
    st, bf, _r = run(c)
    assert st["dof"] == 1
    for b in range(SC.B):
        compare(c, b, st, bf, refs[b], SC.problem_inputs(d, b)[1])
    for dof in (0, -1):
        c = SC.dof_edge_case(shape, dtype, kset, dof)
        st, bf, _r = run(c)
        assert st["dof"] == dof and (st["status"] == 4).all()
        assert np.isnan(st["cov"]).all() and np.isnan(st["reduced_chi2"]).all() and np.isnan(st["conf_sigma"]).all()
        for b, ref in enumerate(SC.reference(c)):  # (the evaluation itself is fine)
            y = SC.problem_inputs(SC.case_data(c), b)[1]
            assert np.abs(bf[b] - ref["best_fit"]).max() <= (1e-10 if dtype == SC.F64 else 8.0 * SC.EPS32 * ref["n"]) * np.abs(y).max()


FAILED_EVALUATION = [SC.CASES[0], next(c for c in SC.CASES if c.set == SC.me_set(SC.F64, 3, 1, 8, 4)),
                     next(c for c in SC.CASES if c.set == SC.me_set(SC.F32, 2, 1, 8))]


@pytest.mark.parametrize("c", FAILED_EVALUATION, ids=ids(FAILED_EVALUATION))
def test_a_failed_evaluation_among_good_problems(c):
    # exp(-t / tau) with a small negative tau overflows (tests/test_gpu_more.py: a failed evaluation like the reference's):
    # that problem reports status 4 and NaN, the others are bit for bit what a batch without it gives
    d = SC.case_data(c)
    bad, good = 2, [0, 1, 3, 4]
    alpha = d["alpha"].copy()
    alpha[bad, 0] = -0.01
    with make_handle(c) as bp:
        bp.set_params(alpha)
        assert (np.asarray(bp.status()) != 0).tolist() == [b == bad for b in range(SC.B)]
        st, bf = bp.statistics(), bp.best_fit()
    with make_handle(c, rows=good) as bp:
        bp.set_params(alpha[good])
        st4, bf4 = bp.statistics(), bp.best_fit()
    assert st["status"].tolist() == [4 if b == bad else 0 for b in range(SC.B)]
    assert np.isnan(st["cov"][bad]).all() and np.isnan(st["reduced_chi2"][bad]) and np.isnan(st["conf_sigma"][bad]).all()
    for k in ("cov", "reduced_chi2", "conf_sigma", "status"):
        assert np.array_equal(st[k][good], st4[k]), k
    assert np.array_equal(bf[good], bf4)
    refs = SC.reference(c)  # (alpha of the good problems is the case's own)
    for i, b in enumerate(good):
        compare(c, i, st4, bf4, refs[b], SC.problem_inputs(d, b)[1], label=" (without problem %d)" % bad)


SIGMA_OFF = [SC.CASES[0], SC.PER_PROBLEM_CASES[1], SC.PER_PROBLEM_CASES[2], next(c for c in SC.CASES if c.set == SC.gen_set(SC.F64))]


@pytest.mark.parametrize("c", SIGMA_OFF, ids=ids(SIGMA_OFF))
def test_statistics_without_confidence_sigma(c):
    d = SC.case_data(c)
    with make_handle(c) as bp:
        bp.set_params(d["alpha"])
        st = bp.statistics()
        st0 = bp.statistics(want_confidence_sigma=False)
    assert st0["conf_sigma"] is None and (st["status"] == 0).all()
    for k in ("cov", "reduced_chi2", "status"):
        assert np.array_equal(st[k], st0[k]), k


DEVICE_POINTERS = [next(c for c in SC.CASES if c.set == SC.me_set(SC.F64, 2, 1, 12)), SC.PER_PROBLEM_CASES[1],
                   next(c for c in SC.CASES if c.set == SC.me_set(SC.F64, 3, 1, 8, 4) and c.m == 1281),
                   next(c for c in SC.CASES if c.set == SC.blk_me_set(SC.F32, 2, 1))]


@pytest.mark.parametrize("c", DEVICE_POINTERS, ids=ids(DEVICE_POINTERS))
def test_device_pointer_outputs_equal_the_host_run_and_stay_inside_their_extent(c):
    # handle and outputs are torch tensors (tests/test_gpu_more.py: device-pointer mode); m does not fill the set, and every
    # output has guard words behind its extent
    import ctypes as C

    import torch
    d = SC.case_data(c)
    st_h, bf_h, _r = run(c)
    dev = torch.device("cuda", 0)
    to = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)  # noqa: E731
    with make_handle(c, x=to(d["x"]), Y=to(d["Y"]), w=to(d["w"])) as bp:
        assert bp.device_mode
        bp.set_params(to(d["alpha"]))
        st_d, bf_d = bp.statistics(), bp.best_fit()
        for k in ("cov", "reduced_chi2", "conf_sigma", "status"):
            assert isinstance(st_d[k], torch.Tensor) and st_d[k].is_cuda
            assert np.array_equal(st_d[k].cpu().numpy(), st_h[k]), k
        assert np.array_equal(bf_d.cpu().numpy(), bf_h)
        # the same calls into buffers with 64 guard words behind each extent
        T = torch.float64 if c.dtype == SC.F64 else torch.float32
        k, guard = st_h["cov"].shape[1], 64
        sizes = dict(cov=(SC.B * k * k, T), chi2=(SC.B, torch.float64), sigma=(SC.B * c.m, T), status=(SC.B, torch.int32),
                     best_fit=(SC.B * c.m, T))
        buf = {name: torch.full((n + guard,), -77, dtype=t, device=dev) for name, (n, t) in sizes.items()}
        ptr = lambda name: C.c_void_p(buf[name].data_ptr())  # noqa: E731
        with torch.cuda.stream(bp._tstream):
            assert bp.lib.vp_statistics(bp._h, ptr("cov"), ptr("chi2"), ptr("sigma"), ptr("status")) == 0
            assert bp.lib.vp_best_fit(bp._h, ptr("best_fit")) == 0
        bp.synchronize()
        torch.cuda.synchronize()
        host = dict(cov=st_h["cov"], chi2=st_h["reduced_chi2"], sigma=st_h["conf_sigma"], status=st_h["status"], best_fit=bf_h)
        for name, (n, _t) in sizes.items():
            got = buf[name].cpu().numpy()
            assert np.array_equal(got[:n], host[name].reshape(-1)), name
            assert (got[n:] == -77).all(), "%s: written beyond its extent" % name


@pytest.mark.parametrize("c", SC.FIT_CASES, ids=ids(SC.FIT_CASES))
def test_statistics_after_a_fit(c):
    # the cached C, cost and status a fit leaves are what the statistics read: against the oracle at the FITTED alpha, for
    # the problems the device reports successful (the oracle's own fits all succeed: tests/test_stats_cases_host.py)
    d = SC.case_data(c)
    with make_handle(c) as bp:
        alpha, coef, rep = bp.fit(SC.fit_guess(c))
        st, bf = bp.statistics(), bp.best_fit()
        assert np.array_equal(np.asarray(bp.params()), alpha)
    ok = np.asarray(rep["termination"]) > 0
    assert ok.sum() >= 4, rep["termination"]
    assert (st["status"][ok] == 0).all()
    for b in np.flatnonzero(ok):
        x, y, w = SC.problem_inputs(d, b)
        ref = SC.reference_at(d["model"], x, y, w, alpha[b].astype(np.float64), c.dtype)
        compare(c, b, st, bf, ref, y, label=" (fitted)")
