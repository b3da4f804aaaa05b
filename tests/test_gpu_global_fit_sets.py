"""The global-fit kernels (several right-hand sides sharing one parameter vector: factor, streaming, cooperative and LM step
kernels of vp_mrhs.hpp) of EVERY compiled kernel set that carries them, against the oracle (tests/mrhs_cases.py holds the
table and the references; tests/test_mrhs_cases_host.py checks the table against the registry and the conditions on its
inputs on the CPU).

Every case first asserts, through vp_debug_kernel_set, that its handle runs on the set the case names, and after every call,
through vp_debug_last_global, that the launches were the ones the case names: waves per problem of the factor and step
kernels, the kernel of the pass over the data columns and its workgroups per problem.  No problem and no column is left out
of a comparison; the 1025 problems of class C are all compared, each with the oracle's result for its distinct problem.

fp64 bounds are those of test_gpu_mrhs.py: evaluation 1e-10, objective 1e-8, parameters 1e-6, trajectory 1e-6 over the leading
evaluations; the trait-level calls against the fused one as test_gpu_parity._check_eval.  fp32 bounds are measured on the
case: FP32_UNIT_MARGIN x max(error of numpy's own fp32 evaluation, eps32 cond(W Phi)) for the evaluation, problem by problem
for C, r and J, over the case for the cost; for the fit the excess objective (F(alpha) - F*) / F* under the fp64 oracle's
cost F, held against FP32_UNIT_MARGIN x max(the same figure of the reference algorithm run in fp32, the fp32 default ftol).

Largest error-to-bound ratios, MI355X (each line prints with `pytest -s`):
  f32 best fit       0.3       A-S3-B5-me2o-m2048-f32@me2o-f32-R32W1
  f32 eval C         0.12      A-S3-B5-me5o-m128-f32-noise1e-05@me5o-f32-R2W1
  f32 eval J         0.37      A-S3-B5-me2o-m1024-f32@me2o-f32-R16W1
  f32 eval cost      0.58      A-S3-B5-me2o-m128-f32@me2o-f32-R2W1
  f32 eval r         0.17      A-S3-B5-me2o-m2048-f32@me2o-f32-R32W1
  f32 fit excess     0.43      A-S3-B5-me5o-m128-f32-noise1e-05@me5o-f32-R2W1
  f32 state cost     0.00029   B-S9-B5-me2o-m2047-f32-w-nu@me2o-f32-R32W1
  f64 best fit       2.7e-05   A-S3-B5-me1o-m2048-f64@me1o-f64-R32W1
  f64 eval C         0.00098   A-S3-B5-me3o_wide-m2048-f64@me3o-f64-R32W1
  f64 eval J         0.009     A-S3-B5-me2o-m2048-f64@me2o-f64-R32W1
  f64 eval cost      0.00062   C-S2-B1025-me1o-m130-f64@me1o-f64-R8W1
  f64 eval r         0.00022   A-S3-B5-me3o_wide-m2048-f64@me3o-f64-R32W1
  f64 fit alpha      0.018     A-S3-B5-me3o_wide-m128-f64@me3o-f64-R2W1
  f64 fit objective  4.7e-06   C-S2-B1025-me1o-m130-f64@me1o-f64-R8W1
  f64 fit traj       4.6e-08   A-S3-B5-rate3o-m128-f64@rt433-f64-R2W1
  f64 state cost     4.8e-07   B-S9-B5-rate1-m127-f64-w-nu@rt111-f64-R2W1
(eval: C, r, J, cost of the fused evaluation; fit: the captured graph against the oracle, traj the leading trial points and
costs of fit_trace; state cost: 1/2 |residuals()|^2 against the reported objective; best fit: w (y - best_fit()) against
residuals().  FP32_UNIT_MARGIN stays 8.)"""
import numpy as np
import pytest

import fit_cases as FC
import mrhs_cases as MC
import stats_cases as SC
import varpro_amd as vp

pytestmark = pytest.mark.gpu
F32_SCALE = SC.EPS32 / SC.EPS64  # an fp64 bound on an agreement to rounding, restated for fp32
TOL = 1e-10  # test_gpu_mrhs.TOL


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _ratio(gc, quantity, value):
    print("ratio %s %-12s %.3e  %s" % ("f64" if gc.case.dtype == SC.F64 else "f32", quantity, value, MC.gcase_id(gc)))


def make_handle(gc, inp):
    bp = vp.BatchProblem(inp["model"], inp["Y"], x=inp["x"], weights=inp["w"])
    got = bp.kernel_set()
    assert got == gc.case.set, "%s runs on %s" % (MC.gcase_id(gc), SC.set_name(got))
    assert bp.last_global_launch() == MC.record(gc)
    return bp


def _eval_check(gc, got, keys):
    """every problem of an evaluation against the oracle's result for its distinct problem; returns the largest ratios"""
    c, d, ref = gc.case, MC.case_data(gc), MC.oracle_evaluate(gc)
    assert (got["status"] == 0).all() and (ref["status"] == 0).all()
    Yw = [MC.weighted_data(d, b) for b in range(MC.NB)]
    J0 = np.zeros_like(ref["J"][0])
    errs = [MC.eval_errors(dict(C=got["C"][i], r=got["r"][i], J=got["J"][i] if "J" in keys else J0 + ref["J"][i % MC.NB],
                                cost=got["cost"][i]), ref, i % MC.NB, Yw[i % MC.NB]) for i in range(gc.B)]
    if c.dtype == SC.F64:
        for k in keys:
            worst = max(e[k] for e in errs)
            _ratio(gc, "eval " + k, worst / TOL)
            assert worst <= TOL, (k, worst)
        return
    bounds, per = MC.fp32_eval_bounds(gc), MC.fp32_eval_bounds_per_problem(gc)
    for k in keys:
        if k == "cost":  # one problem's cost is one draw of the rounding of its residuals: held against the case's bound
            worst = max(e[k] for e in errs)
            _ratio(gc, "eval cost", worst / bounds["cost"])
            assert worst <= bounds["cost"], (worst, bounds["cost"])
            continue
        for i, e in enumerate(errs):
            assert e[k] <= per[i % MC.NB][k], (k, i, e[k], per[i % MC.NB][k])
        _ratio(gc, "eval " + k, max(e[k] / per[i % MC.NB][k] for i, e in enumerate(errs)))


@pytest.mark.parametrize("gc", MC.CASES, ids=MC.IDS)
def test_evaluation_and_stacked_jacobian_of_every_set(gc):
    inp, d = MC.handle_inputs(gc), MC.case_data(gc)
    scale = 1.0 if gc.case.dtype == SC.F64 else F32_SCALE
    with make_handle(gc, inp) as bp:
        got = bp.evaluate(inp["alpha"])
        assert bp.last_global_launch() == MC.record(gc, evaluated=(True, True))
        _eval_check(gc, got, MC.EVAL_KEYS)
        # without the Jacobian: the cooperative output kernel's other instantiation on the fp64 R = 32 sets
        noj = bp.evaluate(inp["alpha"], want_jacobian=False)
        assert bp.last_global_launch() == MC.record(gc, evaluated=(True, False))
        assert noj["J"] is None
        _eval_check(gc, noj, ("C", "r", "cost"))
        # the trait-level calls against the fused one, as test_gpu_parity._check_eval (fp32: its figures times eps32 / eps64)
        bp.set_params(inp["alpha"])
        assert bp.last_global_launch() == MC.record(gc, evaluated=(True, False))
        ymax = max(np.abs(MC.weighted_data(d, b)).max() for b in range(MC.NB))
        assert np.abs(_f64(bp.residuals()) - _f64(got["r"])).max() <= 1e-13 * scale * ymax
        assert bp.last_global_launch() == MC.record(gc, evaluated=(True, False))  # (the cached residuals: no launch)
        assert np.array_equal(np.asarray(bp.jacobian()), got["J"])
        assert bp.last_global_launch() == MC.record(gc, evaluated=(False, True))
        assert np.abs(_f64(bp.linear_coefficients()) - _f64(got["C"])).max() <= 1e-11 * scale * np.abs(got["C"]).max()
        assert np.abs(np.asarray(bp.cost()) - got["cost"]).max() <= 1e-11 * scale * max(got["cost"].max(), ymax ** 2 * 1e-6)


def _state_after_fit(gc, bp, inp, alpha, C, rep):
    """handle state after a global fit == state at the returned parameters"""
    c, d, n = gc.case, MC.case_data(gc), len(SC.SHAPES[gc.case.shape].kinds)
    assert np.array_equal(np.asarray(bp.params()), alpha)
    assert np.array_equal(np.asarray(bp.linear_coefficients()), C)
    r = _f64(bp.residuals())
    assert bp.last_global_launch() == MC.record(gc, evaluated=(True, False), fitted=True)
    cost = 0.5 * (r ** 2).sum(1)
    ysq = np.array([float((MC.weighted_data(d, b) ** 2).sum()) for b in range(MC.NB)])[inp["index"]]
    if c.dtype == SC.F64:  # test_gpu_mrhs.test_mrhs_fit_matches_oracle's bound
        rel = np.abs(cost - rep["objective"]) / np.maximum(rep["objective"], 1e-12 * ysq)
        _ratio(gc, "state cost", rel.max() / 1e-9)
        assert (rel <= 1e-9).all(), rel.max()
    else:  # fp32, first order as test_gpu_fit_sets._state_after_fit: relative 2 n eps32 |y| / |r| on either side
        rel = np.abs(cost - rep["objective"]) / rep["objective"]
        bound = 4.0 * n * SC.EPS32 * np.sqrt(ysq / (2.0 * rep["objective"]))
        _ratio(gc, "state cost", (rel / bound).max())
        assert (rel <= bound).all(), (rel / bound).max()
    # best_fit() + residuals = data, in the residuals' own (weighted) coordinates: w (y - best fit) = r.  The two sides are
    # rounded independently, so the identity holds to the SUM of the bounds tests/test_gpu_stats_sets.py holds each side to
    # against the oracle: tol max |y| for the best fit, times the weight it is multiplied by here, and 2 tol max |y| for the
    # residuals (tol = stats_cases' best-fit tolerance: 1e-10 in fp64, 8 eps32 n in fp32).  (Held against tol max |y| alone,
    # which forgets the residuals' own rounding and the weight, one fp32 weighted case came to 1.012 of it.)
    bf = _f64(bp.best_fit())
    assert bp.last_global_launch() == MC.record(gc, evaluated=(True, False), fitted=True)
    tol = SC.TOL64["best_fit"] if c.dtype == SC.F64 else 8.0 * SC.EPS32 * n
    worst = 0.0
    for i in range(gc.B):
        _x, Y, w = MC.problem_inputs(d, i % MC.NB)
        rw = (Y - bf[i]) * (1.0 if w is None else w)
        wmax = 1.0 if w is None else float(np.abs(w).max())
        worst = max(worst, np.abs(rw.reshape(-1) - r[i]).max() / ((wmax + 2.0) * np.abs(Y).max()))
    _ratio(gc, "best fit", worst / tol)
    assert worst <= tol, worst


def _compare_fit(gc, inp, alpha, rep):
    """the same success class as the oracle, then the fp64 bounds of test_gpu_mrhs or the fp32 excess objective"""
    c, ref, idx = gc.case, MC.oracle_fit(gc), inp["index"]
    assert (ref["termination"] > 0).all(), ref["termination"]
    assert ((rep["termination"] > 0) == (ref["termination"][idx] > 0)).all(), rep["termination"]
    if c.dtype == SC.F64:
        rel_o = np.abs(rep["objective"] - ref["objective"][idx]) / ref["objective"][idx]
        rel_a = (np.abs(alpha - ref["alpha"][idx]) / np.abs(ref["alpha"][idx]).max(1, keepdims=True)).max(1)
        _ratio(gc, "fit objective", rel_o.max() / 1e-8)
        _ratio(gc, "fit alpha", rel_a.max() / 1e-6)
        assert (rel_o <= 1e-8).all(), rel_o.max()
        assert (rel_a <= 1e-6).all(), rel_a.max()
        return
    ref32, ftol = MC.oracle_fit_f32_excess(gc), FC.device_ftol32()
    cost = {}  # (equal parameters of repeated problems: one oracle evaluation)
    for i in range(gc.B):
        key = (int(idx[i]), alpha[i].tobytes())
        if key not in cost:
            cost[key] = MC.oracle_cost(gc, int(idx[i]), alpha[i])
    excess = np.array([(cost[(int(idx[i]), alpha[i].tobytes())] - ref["objective"][idx[i]]) / ref["objective"][idx[i]] for i in range(gc.B)])
    bound = SC.FP32_UNIT_MARGIN * np.maximum(ref32, ftol)[idx]
    _ratio(gc, "fit excess", (excess / bound).max())
    assert (excess <= bound).all(), (excess / bound).max()


@pytest.mark.parametrize("gc", MC.CASES, ids=MC.IDS)
def test_global_fit_of_every_set_against_the_oracle(gc):
    inp = MC.handle_inputs(gc)
    with make_handle(gc, inp) as bp:
        alpha, C, rep = bp.fit(inp["guess"])  # (the captured graph)
        assert bp.last_global_launch() == MC.record(gc, fitted=True)
        _compare_fit(gc, inp, alpha, rep)
        _state_after_fit(gc, bp, inp, alpha, C, rep)


TRACED = [gc for gc in MC.CASES if gc.cls == "A"]


@pytest.mark.parametrize("gc", TRACED, ids=[MC.gcase_id(gc) for gc in TRACED])
def test_global_fit_without_the_graph_and_its_trajectory(gc):
    inp, ref = MC.handle_inputs(gc), MC.oracle_fit(gc)
    q = inp["guess"].shape[1]
    with make_handle(gc, inp) as bp:
        alpha, C, rep, tr = bp.fit_trace(inp["guess"], max_rows=12)  # (plain launches: a trace keeps the graph out)
        assert bp.last_global_launch() == MC.record(gc, fitted=True)
        _compare_fit(gc, inp, alpha, rep)
        if gc.case.dtype == SC.F64:  # test_gpu_mrhs.test_mrhs_fit_matches_oracle: the leading evaluations to 1e-6
            worst = 0.0
            for i in range(gc.B):
                tr_ref, rows = ref["trace"][i % MC.NB], 0
                for j in range(min(5, len(tr_ref), int(rep["n_evals"][i]))):
                    if tr_ref[j, q] < 1e-6 * tr_ref[0, q]:
                        break
                    ea = np.abs(tr[i, j, :q] - tr_ref[j, :q]).max() / np.abs(tr_ref[j, :q]).max()
                    ef = abs(tr[i, j, q] - tr_ref[j, q]) / tr_ref[j, q]
                    worst = max(worst, ea, ef)
                    assert ea <= 1e-6 and ef <= 1e-6, (i, j, tr[i, j], tr_ref[j])
                    rows += 1
                assert rows >= 3, (i, rows)
            _ratio(gc, "fit traj", worst / 1e-6)
        _state_after_fit(gc, bp, inp, alpha, C, rep)
