"""The evaluation kernel (coefficients, residuals, Kaufman Jacobian, cost), the wave fit kernel and the slot fit kernel of EVERY
compiled kernel set (tests/fit_cases.py holds the table and the references; tests/test_fit_cases_host.py checks the table
against the registry and the conditions on its inputs on the CPU).

Every case first asserts, through vp_debug_kernel_set, that its handle runs on the set the case names, and after every fit,
through vp_debug_last_fit, that the launch was the kernel and the padding variant the case names: a slot-kernel launcher that
hands the batch to the wave kernel cannot pass for the slot kernel.  No problem is left out of a comparison.

fp64 bounds are those of test_gpu_parity (_check_eval, imported), test_gpu_rt_sizes and test_gpu_slot_kernel.  fp32 bounds are
measured on the case: FP32_UNIT_MARGIN x max(error of numpy's own fp32 evaluation, eps32 cond(W Phi)) for the evaluation, problem
by problem for C, r and J, over the case's five problems for the cost (one problem's cost error is one draw: 1.6 x the
per-problem bound on B-me2o-m127-f32, 0.58 x the case's); for
the fit the excess objective (F(alpha) - F*) / F* under the fp64 oracle's cost F, held against FP32_UNIT_MARGIN x max(the
same figure of the reference algorithm run in fp32, the fp32 default ftol).

Largest error-to-bound ratios, MI355X (each line prints with `pytest -s`):
  f32 eval C         0.15     G-mixed5-m302-f32@generic-f32
  f32 eval J         0.39     A-me2o-m512-f32@me2o-f32-R8W1
  f32 eval cost      0.58     B-me2o-m127-f32-nu@me2o-f32-R2W1
  f32 eval cost/1    1.6      B-me2o-m127-f32-nu@me2o-f32-R2W1
  f32 eval r         0.18     G-mixed5-m302-f32@generic-f32
  f32 fit excess     0.16     A-me5o-m128-f32-noise1e-05@me5o-f32-R2W1
  f32 slots C        0        
  f32 state cost     0.022    B-me2o-m127-f32-nu@me2o-f32-R2W1
  f64 eval C         0.00075  A-me3o_wide-m1280-f64@me3o-f64-R20W1
  f64 eval J         0.005    A-me3o_wide-m2048-f64@me3o-f64-R8W4
  f64 eval cost      0.0006   L-rate1o-m1025-f64@rt211-f64-blk
  f64 eval r         0.00013  C-me3o_wide-m1282-f64-w@me3o-f64-R8W4
  f64 fit C          0.2      L-me5o-m300-f64@me5o-f64-blk
  f64 fit alpha      0.079    L-me5o-m300-f64@me5o-f64-blk
  f64 fit objective  4.8e-06  B-me1o-m127-f64-nu@me1o-f64-R2W1
  f64 slots C        0        
  f64 state cost     4.7e-09  C-rate1o-m130-f64-w@rt211-f64-R16W1
(eval: C, r, J, cost of the fused evaluation, cost/1 the cost against the per-problem bound, printed only -- fp64 over 1e-10 of the scale, J without _check_eval's floor; fit: the wave kernel
against the oracle; state cost: 1/2 |residuals()|^2 against the reported objective; slots C: slot kernel against wave kernel,
everything else there being bit-equal.)
The fp32 bounds that the fp64 tests have no counterpart for are this file's own: the state cost (first order, 4 n eps32 |y| /
|r|, see _state_after_fit), and the trait-level calls and the summary at the fp64 figures times eps32 / eps64.
"""
import numpy as np
import pytest

import fit_cases as FC
import stats_cases as SC
import varpro_amd as vp
from test_gpu_parity import _check_eval
from test_gpu_stats_sets import make_handle

pytestmark = pytest.mark.gpu
SLOT_CASES = [fc for fc in FC.FIT_CASES if fc.slots is not None]
ids = lambda cases: [FC.fit_case_id(fc) for fc in cases]  # noqa: E731
F32_SCALE = SC.EPS32 / SC.EPS64  # an fp64 bound on an agreement to rounding, restated for fp32


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _ratio(fc, quantity, value):
    print("ratio %s %-12s %.3e  %s" % ("f64" if fc.case.dtype == SC.F64 else "f32", quantity, value, FC.fit_case_id(fc)))


# ---- evaluation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fc", FC.FIT_CASES, ids=FC.IDS)
def test_evaluation_and_kaufman_jacobian_of_every_kernel_set(fc):
    c = fc.case
    d, ref = SC.case_data(c), FC.oracle_evaluate(c)
    yws = [y if w is None else y * w for _x, y, w in (SC.problem_inputs(d, b) for b in range(SC.B))]
    with make_handle(c) as bp:
        if c.dtype == SC.F64:
            got = _check_eval(d["model"], d["x"], d["Y"], d["alpha"], d["w"], bp=bp)
            errs = [FC.eval_errors({k: got[k][b] for k in FC.EVAL_KEYS}, ref, b, np.abs(yws[b]).max(), float(yws[b] @ yws[b]))
                    for b in range(SC.B)]
            for k in FC.EVAL_KEYS:  # (J: without the floor 1e-13 max |W D_k c| of _check_eval, so this ratio may pass 1)
                _ratio(fc, "eval " + k, max(e[k] for e in errs) / 1e-10)
            return
        got = bp.evaluate(d["alpha"])
        assert (got["status"] == 0).all() and (ref["status"] == 0).all()
        errs = [FC.eval_errors({k: got[k][b] for k in FC.EVAL_KEYS}, ref, b, np.abs(yws[b]).max(), float(yws[b] @ yws[b]))
                for b in range(SC.B)]
        # C, r, J problem by problem.  The cost 1/2 |r|^2 of ONE problem is one draw of the rounding of its residuals, not a
        # bound of it (stats_cases.py on chi2, the same quantity over dof): it is held against the case's largest e_np32
        bounds, per = FC.fp32_eval_bounds(c), FC.fp32_eval_bounds_per_problem(c)
        for k in ("C", "r", "J"):
            for b in range(SC.B):
                assert errs[b][k] <= per[b][k], (k, b, errs[b][k], per[b][k])
            _ratio(fc, "eval " + k, max(errs[b][k] / per[b][k] for b in range(SC.B)))
        e = max(x["cost"] for x in errs)
        _ratio(fc, "eval cost", e / bounds["cost"])
        _ratio(fc, "eval cost/1", max(errs[b]["cost"] / per[b]["cost"] for b in range(SC.B)))  # (per problem: printed only)
        assert e <= bounds["cost"], (e, bounds["cost"])
        # the trait-level calls against the fused one, as _check_eval: its fp64 figures scaled by eps32 / eps64
        bp.set_params(d["alpha"])
        ymax = max(np.abs(y).max() for y in yws)
        assert np.abs(_f64(bp.residuals()) - _f64(got["r"])).max() <= 1e-13 * F32_SCALE * ymax
        assert np.array_equal(np.asarray(bp.jacobian()), got["J"])
        assert np.abs(_f64(bp.linear_coefficients()) - _f64(got["C"])).max() <= 1e-11 * F32_SCALE * np.abs(got["C"]).max()
        assert np.abs(np.asarray(bp.cost()) - got["cost"]).max() <= 1e-11 * F32_SCALE * max(got["cost"].max(), ymax ** 2 * 1e-6)


# ---- the wave kernel against the oracle ------------------------------------------------------------------------------------
def _state_after_fit(fc, bp, alpha, C, rep, yws):
    """handle state after a fit == state at the final parameters; summary counts exact"""
    c, n = fc.case, len(SC.SHAPES[fc.case.shape].kinds)
    assert np.array_equal(np.asarray(bp.params()), alpha)
    assert np.array_equal(np.asarray(bp.linear_coefficients()), C)
    r = _f64(bp.residuals())
    cost = 0.5 * (r ** 2).sum(1)
    ysq = np.array([float(y @ y) for y in yws])
    if c.dtype == SC.F64:  # test_gpu_parity._check_fit's bound
        rel = np.abs(cost - rep["objective"]) / np.maximum(rep["objective"], 1e-12 * ysq)
        _ratio(fc, "state cost", rel.max() / 1e-5)
        assert np.median(rel) <= 1e-12 and np.quantile(rel, 0.9) <= 1e-9 and rel.max() <= 1e-5, rel
    else:
        # fp32, first order: every r_i = y_i - sum_j phi_ij c_j carries n eps32 |y_i|, so 1/2 |r|^2 moves by |r| n eps32 |y|,
        # relative 2 n eps32 |y| / |r|; both the reported objective and the recomputed one carry it
        rel = np.abs(cost - rep["objective"]) / rep["objective"]
        bound = 4.0 * n * SC.EPS32 * np.sqrt(ysq / (2.0 * rep["objective"]))
        _ratio(fc, "state cost", (rel / bound).max())
        assert (rel <= bound).all(), (rel, bound)
    s = bp.summary()
    assert s[1] == (rep["termination"] > 0).sum() and s[2] == (rep["termination"] <= 0).sum()
    assert s[3] == rep["n_evals"].sum()
    assert abs(s[0] - rep["objective"].sum()) <= (1e-12 if c.dtype == SC.F64 else 1e-12 * F32_SCALE) * rep["objective"].sum()


@pytest.mark.parametrize("fc", FC.FIT_CASES, ids=FC.IDS)
def test_wave_kernel_fit_against_the_oracle(fc):
    c = fc.case
    d, g, ref = SC.case_data(c), SC.fit_guess(c), FC.oracle_fit(c)
    q = g.shape[1]
    yws = [y if w is None else y * w for _x, y, w in (SC.problem_inputs(d, b) for b in range(SC.B))]
    with make_handle(c) as bp:
        assert bp.last_fit_kernel() == (0, 0, 0, 0)
        bp.set_fit_kernel("wave")
        alpha, C, rep, tr = bp.fit_trace(g, max_rows=16)
        assert bp.last_fit_kernel() == fc.wave
        assert (ref["termination"] > 0).all(), ref["termination"]
        assert (rep["termination"] > 0).all(), rep["termination"]
        if c.dtype == SC.F64:
            for b in range(SC.B):
                tr_ref, rows = ref["trace"][b], 0
                f0 = tr_ref[0, q]
                for i in range(min(6, len(tr_ref), int(rep["n_evals"][b]))):
                    if tr_ref[i, q] < 1e-6 * f0:
                        break  # inside the rounding-noise regime of a (near) perfect fit
                    got, want = tr[b, i], tr_ref[i]
                    assert np.abs(got[:q] - want[:q]).max() <= 1e-8 * np.abs(want[:q]).max(), (b, i, got, want)
                    assert abs(got[q] - want[q]) <= 1e-8 * abs(want[q]), (b, i, got, want)
                    rows += 1
                assert rows >= 3, (b, rows)
            rel_o = np.abs(rep["objective"] - ref["objective"]) / ref["objective"]
            rel_a = (np.abs(alpha - ref["alpha"]) / np.abs(ref["alpha"]).max(1, keepdims=True)).max(1)
            rel_c = (np.abs(C - ref["C"]) / np.abs(ref["C"]).max(1, keepdims=True)).max(1)
            _ratio(fc, "fit objective", rel_o.max() / 1e-8)
            _ratio(fc, "fit alpha", rel_a.max() / 1e-5)
            _ratio(fc, "fit C", rel_c.max() / 1e-6)
            assert (rel_o <= 1e-8).all(), rel_o
            assert (rel_a <= 1e-5).all(), rel_a
            assert (rel_c <= 1e-6).all(), rel_c
        else:
            ref32, ftol = FC.oracle_fit_f32_excess(c), FC.device_ftol32()
            excess = np.array([(FC.oracle_cost(c, b, alpha[b]) - ref["objective"][b]) / ref["objective"][b] for b in range(SC.B)])
            bound = SC.FP32_UNIT_MARGIN * np.maximum(ref32, ftol)
            _ratio(fc, "fit excess", (excess / bound).max())
            assert (excess <= bound).all(), (excess, ref32, ftol)
        _state_after_fit(fc, bp, alpha, C, rep, yws)


# ---- the slot kernel against the wave kernel -------------------------------------------------------------------------------
def _equal_fits(fc, wave, slots):
    (a0, c0, r0, t0), (a1, c1, r1, t1) = wave, slots
    assert np.array_equal(r0["termination"], r1["termination"])
    assert np.array_equal(r0["n_evals"], r1["n_evals"])
    assert np.array_equal(r0["objective"], r1["objective"], equal_nan=True)
    assert np.array_equal(a0, a1)
    assert np.array_equal(t0, t1, equal_nan=True)
    assert np.array_equal(np.isnan(c0), np.isnan(c1))
    dc = np.nanmax(np.abs(_f64(c0) - _f64(c1))) / np.nanmax(np.abs(c0))
    tol = 1e-13 * (1.0 if fc.case.dtype == SC.F64 else F32_SCALE)
    _ratio(fc, "slots C", dc / tol)
    assert dc <= tol, dc


@pytest.mark.parametrize("fc", SLOT_CASES, ids=ids(SLOT_CASES))
def test_slot_kernel_equals_wave_kernel_on_every_set_that_has_one(fc):
    c, g, out = fc.case, SC.fit_guess(fc.case), {}
    for kernel in ("wave", "slots"):
        with make_handle(c) as bp:
            bp.set_fit_kernel(kernel)
            out[kernel] = bp.fit_trace(g, max_rows=16)
            assert bp.last_fit_kernel() == (fc.wave if kernel == "wave" else fc.slots)
    if fc.slots[0] != FC.SLOTS:
        # weights, per-problem grids, a set whose slots do not fit the LDS: launch_fit2 handed the batch to the wave kernel
        # and says so (asserted above) -- nothing to compare
        assert fc.slots == fc.wave and (c.weights is not None or c.grid == "per" or not FC.slots_fit_lds(c.set))
        return
    assert fc.slots == (FC.SLOTS, FC.padding_class(c.m, c.set[5], c.set[6]), 0, 0)
    _equal_fits(fc, out["wave"], out["slots"])


@pytest.mark.parametrize("fc", FC.REFILL_CASES, ids=ids(FC.REFILL_CASES))
def test_slot_kernel_queue_refill_beyond_the_double_exponential(fc):
    # 700 problems: more than one wave's slots, so finished slots pull the rest from the queue
    c = fc.case
    d = FC.refill_data(c)
    out = {}
    for kernel in ("wave", "slots"):
        with vp.BatchProblem(d["model"], d["Y"], x=d["x"]) as bp:
            assert bp.kernel_set() == c.set
            bp.set_fit_kernel(kernel)
            out[kernel] = bp.fit_trace(d["guess"], max_rows=8)
            assert bp.last_fit_kernel() == (fc.wave if kernel == "wave" else fc.slots)
    assert (out["wave"][2]["termination"] > 0).mean() > 0.9
    _equal_fits(fc, out["wave"], out["slots"])
