"""GPU tier of the start-point search (vp_search, varpro_amd/csrc/vp_search.hpp): the shared route -- candidate columns,
orthonormalisation, the MFMA ranking product -- and the candidate loop, against numpy in fp64 (tests/search_cases.py:
``lstsq`` on W Phi for every candidate, cost 1/2 ||r||^2).

fp64 criterion (search_cases.check_fp64): index_out equals numpy's argmin on every problem whose best and second-best
numpy costs differ by more than 8 n m eps |y_w|^2, the dot-product error bound of a score; at most 2 % of the problems may
be excluded by that rule; on every problem the numpy cost of the chosen candidate is <= the numpy minimum + that bound;
cost_out agrees with numpy to contracts.EVALUATION_REL_TOL.  fp32 criterion (check_fp32): the worst-case bound is vacuous
there, so the excess of the chosen candidate's numpy cost over the minimum is held to 8 eps32 |y_w|^2; no index equality.
(m < n: every candidate fits the data exactly, all costs are rounding noise and the gap rule decides nothing -- the 2 % cap
cannot apply there and is the one thing that case does not assert; its cost_out limit carries the floor eps |y_w|^2.)"""
import numpy as np
import pytest

import contracts as K
import search_cases as sc
import varpro_amd as vp
from varpro_amd import _lib, basis

pytestmark = pytest.mark.gpu
TOL = K.EVALUATION_REL_TOL


def _state(bp):
    return dict(params=bp.params(), cost=bp.cost(), r=bp.residuals(), C=bp.linear_coefficients(), status=bp.status())


def _same_state(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in a)


def _consistent(bp, make_fresh, cand, alpha, index, cost, per_problem=False):
    """after the call: alpha_out is the chosen candidate; params() is alpha_out bit for bit; cost() is cost_out;
    residuals() are those of a fresh set_params(alpha_out) bit for bit"""
    B = alpha.shape[0]
    pick = np.maximum(index, 0)
    want = cand[np.arange(B), pick] if per_problem else cand[pick]
    assert np.array_equal(alpha, want.astype(alpha.dtype), equal_nan=True)
    assert np.array_equal(bp.params(), alpha, equal_nan=True)
    assert np.array_equal(bp.cost(), cost, equal_nan=True)
    fresh = make_fresh()
    fresh.set_params(alpha)
    assert np.array_equal(bp.residuals(), fresh.residuals(), equal_nan=True)
    assert np.array_equal(bp.linear_coefficients(), fresh.linear_coefficients(), equal_nan=True)
    assert np.array_equal(bp.status(), fresh.status())
    fresh.close()


# ---- 1. shared route, fp64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("m", [37, 130, 1030])
def test_shared_route_fp64(m, weighted):
    d = sc.base_data(m)
    w = d["w"] if weighted else None
    cand = sc.base_candidates()
    make = lambda: vp.BatchProblem(sc.double_exp_model(d["x"]), d["Y"], x=d["x"], weights=w)  # noqa: E731
    bp = make()
    alpha, index, cost = bp.search(cand)
    cost_np, y2 = sc.base_costs(m, weighted)
    sc.check_fp64(index, cost, cost_np, y2, 3, m, TOL)
    _consistent(bp, make, cand, alpha, index, cost)
    assert (bp.status() == 0).all()
    bp.close()


# ---- 2. shared route, several right-hand sides ----------------------------------------------------------------------------
@pytest.mark.parametrize("m", [37, 130])
def test_shared_route_three_right_hand_sides(m):
    """m = 130: rows of Y_w are 16-byte aligned -- the vector-load variant of the score-matrix kernel"""
    d = sc.base_data(m)
    rng = np.random.default_rng(5)
    Y3 = np.stack([d["Y"], 0.7 * d["Y"] + 1e-2 * rng.standard_normal(d["Y"].shape),
                   1.3 * d["Y"] + 1e-2 * rng.standard_normal(d["Y"].shape)], 1)
    cand = sc.base_candidates()
    mdl = sc.double_exp_model(d["x"])
    make = lambda: vp.BatchProblem(mdl, Y3, x=d["x"], weights=d["w"])  # noqa: E731
    bp = make()
    alpha, index, cost = bp.search(cand)
    cost_np, y2 = sc.numpy_costs(mdl, d["x"], cand, Y3, d["w"])
    sc.check_fp64(index, cost, cost_np, y2, 3, m, TOL)
    # ... and the costs ARE sums over the right-hand sides: the winner of a single column may differ
    one, _ = sc.numpy_costs(mdl, d["x"], cand, Y3[:, 0], d["w"])
    assert cost_np.min(1).sum() > one.min(1).sum()
    _consistent(bp, make, cand, alpha, index, cost)
    bp.close()


# ---- 3. candidate loop ----------------------------------------------------------------------------------------------------
def _loop_case(which):
    m = 37
    d = sc.base_data(m)
    B = d["Y"].shape[0]
    rng = np.random.default_rng(11)
    x, Y, w, cand, per_problem, cap = d["x"], d["Y"], None, sc.base_candidates(), False, 0.02
    if which == "candidates":
        cand = cand[None, :25] * rng.uniform(0.97, 1.03, (B, 25, 2))
        per_problem = True
    elif which == "grid":
        x = d["x"][None, :] + rng.uniform(-0.01, 0.01, (B, m))
    elif which == "weights":
        w = 0.5 + rng.random((B, m))
    elif which == "m<n":
        x, Y, cap = d["x"][:2] + 0.5, d["Y"][:, :2], None
    return x, Y, w, cand, per_problem, cap


@pytest.mark.parametrize("which", ["candidates", "grid", "weights", "m<n"])
def test_candidate_loop(which):
    x, Y, w, cand, per_problem, cap = _loop_case(which)
    m = Y.shape[1]
    mdl = sc.double_exp_model(x if x.ndim == 1 else x[0])
    make = lambda: vp.BatchProblem(mdl, Y, x=x, weights=w)  # noqa: E731
    bp = make()
    alpha, index, cost = bp.search(cand, per_problem=per_problem)
    cost_np, y2 = sc.numpy_costs(mdl, x, cand, Y, w)
    sc.check_fp64(index, cost, cost_np, y2, 3, m, TOL, cap=cap, floor=cap is None)
    _consistent(bp, make, cand, alpha, index, cost, per_problem)
    bp.close()


# ---- 4. the two routes agree ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_the_two_routes_agree(weighted):
    m = 130
    d = sc.base_data(m)
    B = d["Y"].shape[0]
    w = d["w"] if weighted else None
    cand = sc.base_candidates()
    a = vp.BatchProblem(sc.double_exp_model(d["x"]), d["Y"], x=d["x"], weights=w)
    b = vp.BatchProblem(sc.double_exp_model(d["x"]), d["Y"], x=d["x"], weights=w)
    alpha_a, index_a, cost_a = a.search(cand)
    alpha_b, index_b, cost_b = b.search(np.ascontiguousarray(np.broadcast_to(cand, (B,) + cand.shape)), per_problem=True)
    assert np.array_equal(index_a, index_b)
    assert np.array_equal(alpha_a, alpha_b) and np.array_equal(cost_a, cost_b)
    assert _same_state(_state(a), _state(b))
    a.close()
    b.close()


# ---- 5. a device-column model ---------------------------------------------------------------------------------------------
def test_device_column_model():
    d = sc.peaks_data()
    m = d["x"].size
    mdl = sc.peaks_model(d["x"])
    cand = sc.peaks_candidates()
    make = lambda: vp.BatchProblem(mdl, d["Y"], x=d["x"])  # noqa: E731
    bp = make()
    alpha, index, cost = bp.search(cand)
    cost_np, y2 = sc.numpy_costs(mdl, d["x"], cand, d["Y"])
    sc.check_fp64(index, cost, cost_np, y2, 4, m, TOL)
    _consistent(bp, make, cand, alpha, index, cost)
    # the same through the candidate loop (per-problem candidates on a device-column handle)
    lp = make()
    B = d["Y"].shape[0]
    alpha_l, index_l, cost_l = lp.search(np.ascontiguousarray(np.broadcast_to(cand, (B,) + cand.shape)), per_problem=True)
    assert np.array_equal(index, index_l) and np.array_equal(alpha, alpha_l) and np.array_equal(cost, cost_l)
    lp.close()
    bp.close()


# ---- 6. fp32 handle, shared route -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [128, 130, 1030])
def test_shared_route_fp32(m):
    """measured on the device: worst excess / (eps32 |y_w|^2) = 1.16 (m = 128), 3.06 (m = 130), 6.89 (m = 1030); limit 8"""
    d = sc.base_data(m)
    x32, Y32, w32 = d["x"].astype(np.float32), d["Y"].astype(np.float32), d["w"].astype(np.float32)
    cand = sc.base_candidates()
    mdl32 = sc.double_exp_model(x32, np.float32)
    make = lambda: vp.BatchProblem(mdl32, Y32, x=x32, weights=w32)  # noqa: E731
    bp = make()
    alpha, index, cost = bp.search(cand)
    assert alpha.dtype == np.float32 and cost.dtype == np.float64
    # the checker works in fp64 on the ROUNDED data the handle holds
    cost_np, y2 = sc.numpy_costs(sc.double_exp_model(x32.astype(np.float64)), x32.astype(np.float64),
                                 cand.astype(np.float32).astype(np.float64), Y32.astype(np.float64), w32.astype(np.float64))
    sc.check_fp32(index, cost_np, y2)
    _consistent(bp, make, cand, alpha, index, cost)
    bp.close()


# ---- 7. non-finite candidates ---------------------------------------------------------------------------------------------
def test_a_nan_candidate_in_a_shared_set_never_wins():
    m = 37
    d = sc.base_data(m)
    cand = sc.base_candidates()
    with_nan = np.vstack([[[np.nan, 4.0]], cand[:7], [[2.0, np.nan]], cand[7:]])
    bp = vp.BatchProblem(sc.double_exp_model(d["x"]), d["Y"], x=d["x"])
    _a0, index0, cost0 = bp.search(cand)
    _a1, index1, cost1 = bp.search(with_nan)
    assert np.array_equal(index1, np.where(index0 < 7, index0 + 1, index0 + 2))
    assert np.array_equal(cost0, cost1) and (bp.status() == 0).all()
    # no finite candidate at all: every problem gets -1, its candidate 0 and a latched status
    alpha, index, _cost = bp.search(with_nan[:1])
    assert (index == -1).all() and np.array_equal(alpha, np.broadcast_to(with_nan[:1], alpha.shape), equal_nan=True)
    assert (bp.status() != 0).all()
    bp.close()


def test_a_problem_without_a_finite_candidate():
    m = 37
    d = sc.base_data(m)
    B = d["Y"].shape[0]
    cand = np.ascontiguousarray(np.broadcast_to(sc.base_candidates(), (B, 26, 2))).copy()
    bp = vp.BatchProblem(sc.double_exp_model(d["x"]), d["Y"], x=d["x"])
    alpha0, index0, cost0 = bp.search(cand, per_problem=True)
    st0 = bp.status()
    bad = 5
    cand[bad] = np.nan
    cand[bad, 0, 1] = 3.0  # (candidate 0 of that problem: half NaN, recognisable)
    alpha, index, cost = bp.search(cand, per_problem=True)
    st = bp.status()
    assert index[bad] == -1 and np.array_equal(alpha[bad], cand[bad, 0], equal_nan=True) and st[bad] != 0
    others = np.arange(B) != bad
    assert np.array_equal(index[others], index0[others]) and np.array_equal(alpha[others], alpha0[others])
    assert np.array_equal(cost[others], cost0[others]) and np.array_equal(st[others], st0[others]) and (st0 == 0).all()
    bp.close()


# ---- 8. edges -------------------------------------------------------------------------------------------------------------
def test_one_candidate():
    m = 37
    d = sc.base_data(m)
    cand = np.array([[1.5, 7.0]])
    make = lambda: vp.BatchProblem(sc.double_exp_model(d["x"]), d["Y"], x=d["x"])  # noqa: E731
    bp = make()
    alpha, index, cost = bp.search(cand)
    assert (index == 0).all()
    cost_np, y2 = sc.numpy_costs(sc.double_exp_model(d["x"]), d["x"], cand, d["Y"])
    sc.check_fp64(index, cost, cost_np, y2, 3, m, TOL)
    _consistent(bp, make, cand, alpha, index, cost)
    bp.close()


def test_300_candidates_5_problems():
    """several candidate tiles (19 groups of 16, the last one partial), fewer problems than a row tile"""
    m = 130
    d = sc.base_data(m)
    Y = d["Y"][:5]
    cand = vp.candidate_grid(np.linspace(0.4, 3.2, 20), np.linspace(3.6, 12.0, 15))
    assert cand.shape == (300, 2)
    mdl = sc.double_exp_model(d["x"])
    make = lambda: vp.BatchProblem(mdl, Y, x=d["x"])  # noqa: E731
    bp = make()
    alpha, index, cost = bp.search(cand)
    cost_np, y2 = sc.numpy_costs(mdl, d["x"], cand, Y)
    sc.check_fp64(index, cost, cost_np, y2, 3, m, TOL)
    assert index.max() >= 16  # (winners beyond the first tile)
    _consistent(bp, make, cand, alpha, index, cost)
    bp.close()


def test_one_basis_function():
    """n = 1: a single exponential without offset"""
    m = 37
    rng = np.random.default_rng(3)
    x = np.linspace(0, 12.5, m)
    tau = rng.uniform(0.8, 6.0, 33)
    Y = rng.uniform(0.5, 2, (33, 1)) * np.exp(-x[None, :] / tau[:, None]) + 1e-2 * rng.standard_normal((33, m))
    mdl = vp.multi_exponential_model(x, [2.0], offset=False)
    cand = vp.candidate_grid([0.5, 1.0, 1.6, 2.4, 3.5, 5.0, 7.0])
    make = lambda: vp.BatchProblem(mdl, Y, x=x)  # noqa: E731
    bp = make()
    alpha, index, cost = bp.search(cand)
    cost_np, y2 = sc.numpy_costs(mdl, x, cand, Y)
    sc.check_fp64(index, cost, cost_np, y2, 1, m, TOL)
    _consistent(bp, make, cand, alpha, index, cost)
    bp.close()


def test_eight_basis_functions():
    """n = 8 on a generic-shape descriptor (three sine / cosine pairs, a decay, a constant)"""
    d = sc.eight_basis_data()
    m = d["x"].size
    mdl = sc.eight_basis_model(d["x"])
    cand = sc.eight_basis_candidates()
    make = lambda: vp.BatchProblem(mdl, d["Y"], x=d["x"])  # noqa: E731
    bp = make()
    alpha, index, cost = bp.search(cand)
    cost_np, y2 = sc.numpy_costs(mdl, d["x"], cand, d["Y"])
    sc.check_fp64(index, cost, cost_np, y2, 8, m, TOL)
    _consistent(bp, make, cand, alpha, index, cost)
    bp.close()


# ---- 9. device tensors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_problem", [False, True])
def test_device_tensors_in_device_tensors_out(per_problem):
    import torch
    m = 130
    d = sc.base_data(m)
    B = d["Y"].shape[0]
    cand = sc.base_candidates()
    if per_problem:
        cand = np.ascontiguousarray(np.broadcast_to(cand, (B,) + cand.shape))
    host = vp.BatchProblem(sc.double_exp_model(d["x"]), d["Y"], x=d["x"], weights=d["w"])
    alpha_h, index_h, cost_h = host.search(cand, per_problem=per_problem)
    dev = vp.BatchProblem(sc.double_exp_model(d["x"]), torch.tensor(d["Y"], device="cuda"), x=d["x"], weights=d["w"])
    alpha_d, index_d, cost_d = dev.search(torch.tensor(cand, device="cuda"), per_problem=per_problem)
    assert all(torch.is_tensor(t) and t.is_cuda for t in (alpha_d, index_d, cost_d)) and index_d.dtype == torch.int32
    assert np.array_equal(alpha_d.cpu().numpy(), alpha_h) and np.array_equal(index_d.cpu().numpy(), index_h)
    assert np.array_equal(cost_d.cpu().numpy(), cost_h)
    assert np.array_equal(dev.residuals().cpu().numpy(), host.residuals())
    host.close()
    dev.close()


# ---- 10. search, then fit -------------------------------------------------------------------------------------------------
def test_fit_from_search_is_search_then_fit():
    m = 130
    d = sc.base_data(m)
    cand = sc.base_candidates()[:25]
    a = vp.BatchProblem(sc.double_exp_model(d["x"]), d["Y"], x=d["x"])
    b = vp.BatchProblem(sc.double_exp_model(d["x"]), d["Y"], x=d["x"])
    alpha_a, C_a, rep_a = a.fit_from_search(cand)
    start, _index, _cost = b.search(cand)
    alpha_b, C_b, rep_b = b.fit(start)
    assert np.array_equal(alpha_a, alpha_b) and np.array_equal(C_a, C_b)
    for field in ("termination", "n_evals", "objective"):
        assert np.array_equal(rep_a[field], rep_b[field])
    assert (rep_a["termination"] > 0).all()
    a.close()
    b.close()


# ---- 11. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    import ctypes as C
    m = 37
    d = sc.base_data(m)
    cand = sc.base_candidates()
    bp = vp.BatchProblem(sc.double_exp_model(d["x"]), d["Y"], x=d["x"])
    bp.set_params(np.broadcast_to([1.0, 6.0], (bp.B, 2)))
    before = _state(bp)
    out = np.empty((bp.B, 2))
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert bp.lib.vp_search(bp._h, ptr(cand), 0, 0, ptr(out), None, None) == _lib.VP_ERR_INVALID   # K = 0
    assert _same_state(before, _state(bp))
    assert bp.lib.vp_search(bp._h, None, 26, 0, ptr(out), None, None) == _lib.VP_ERR_INVALID        # null cand
    assert _same_state(before, _state(bp))
    assert bp.lib.vp_search(bp._h, ptr(cand), 26, 2, ptr(out), None, None) == _lib.VP_ERR_INVALID   # unknown flag
    assert _same_state(before, _state(bp))
    bp.close()

    # a caller-evaluated handle: the device cannot evaluate the model
    x = d["x"]
    ext = vp.ExternalModel(3, 2, [(0, 0), (1, 1)])
    eb = vp.BatchProblem(ext, d["Y"])
    a0 = np.broadcast_to([1.0, 6.0], (eb.B, 2)).copy()
    Phi = np.stack([np.exp(-x / 1.0), np.exp(-x / 6.0), np.ones_like(x)])[None].repeat(eb.B, 0)
    dPhi = np.stack([Phi[0, 0] * x, Phi[0, 1] * x / 36.0])[None].repeat(eb.B, 0)
    eb.set_params_with_basis(a0, Phi, dPhi)
    before = dict(params=eb.params(), cost=eb.cost())
    with pytest.raises(vp.VarproHipError) as err:
        eb.search(cand)
    assert err.value.code == _lib.VP_ERR_UNSUPPORTED
    assert np.array_equal(eb.params(), before["params"]) and np.array_equal(eb.cost(), before["cost"])
    # ... and between fit_begin and fit_end a search is invalid; the stepped fit goes on as on a twin handle that was never
    # asked (the getters are not legal during a stepped fit: the state is compared through the fit's results)
    twin = vp.BatchProblem(ext, d["Y"])
    twin.set_params_with_basis(a0, Phi, dPhi)
    twin.fit_begin(a0)
    eb.fit_begin(a0)
    with pytest.raises(vp.VarproHipError) as err:
        eb.search(cand)
    assert err.value.code == _lib.VP_ERR_INVALID
    step_e, step_t = eb.fit_step_with_basis(Phi, dPhi), twin.fit_step_with_basis(Phi, dPhi)
    assert np.array_equal(step_e[0], step_t[0]) and np.array_equal(step_e[1], step_t[1]) and step_e[2] == step_t[2]
    end_e, end_t = eb.fit_end(), twin.fit_end()
    assert np.array_equal(end_e[0], end_t[0]) and np.array_equal(end_e[1], end_t[1])
    assert all(np.array_equal(end_e[2][f], end_t[2][f], equal_nan=True) for f in ("termination", "n_evals", "objective"))
    assert np.array_equal(eb.params(), twin.params()) and np.array_equal(eb.cost(), twin.cost(), equal_nan=True)
    twin.close()
    eb.close()
