"""CPU tier of the start-point search (vp_search / BatchProblem.search): the declaration in every binding, the refusal of a
null handle without a device, ``candidate_grid`` and the numpy mirror of the device's ranking (varpro_amd/search.py)."""
import os
import re

import numpy as np
import pytest

import search_cases as sc
import varpro_amd as vp
from varpro_amd import _lib, search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_in_the_header_and_every_binding():
    header = open(os.path.join(ROOT, "include", "varpro_hip.h")).read()
    assert re.search(r"enum \{ VP_SEARCH_PER_PROBLEM = 1 \};", header)
    assert re.search(r"int vp_search\(vp_batch \*h, const void \*cand, int64_t K, int flags,\s*"
                     r"void \*alpha_out, int32_t \*index_out, double \*cost_out\);", header)
    assert "vp_search" in _lib.ABI_SYMBOLS and _lib.VP_SEARCH_PER_PROBLEM == 1
    lib = vp.load_library()
    assert hasattr(lib, "vp_search") and len(lib.vp_search.argtypes) == 7
    rust = open(os.path.join(ROOT, "bindings", "rust", "varpro_hip.rs")).read()
    assert re.search(r"pub fn vp_search\(h: \*mut vp_batch, cand: \*const c_void, k: i64, flags: i32, alpha_out: \*mut c_void,\s*"
                     r"index_out: \*mut i32, cost_out: \*mut f64\) -> i32;", rust)
    assert re.search(r"VP_SEARCH_PER_PROBLEM: i32 = 1;", rust)
    cpp = open(os.path.join(ROOT, "varpro_amd", "cpp", "varpro.hpp")).read()
    assert "vp_search" in cpp and "VP_SEARCH_PER_PROBLEM" in cpp


def test_null_handle_is_refused_without_a_device():
    lib = vp.load_library()
    cand = np.zeros((2, 2))
    assert lib.vp_search(None, cand.ctypes.data, 2, 0, None, None, None) == _lib.VP_ERR_INVALID
    assert b"null handle" in lib.vp_last_error()


def test_candidate_grid_shapes_and_predicate():
    g = vp.candidate_grid([0.5, 1.0, 2.0], [4.0, 8.0])
    assert g.shape == (6, 2) and g.dtype == np.float64
    assert np.array_equal(g[0], [0.5, 4.0]) and np.array_equal(g[1], [0.5, 8.0]) and np.array_equal(g[-1], [2.0, 8.0])
    assert vp.candidate_grid([1.0, 2.0, 3.0]).shape == (3, 1)
    assert vp.candidate_grid(np.linspace(0, 1, 4), [1, 2], (5.0, 6.0, 7.0)).shape == (24, 3)
    t = [1.0, 2.0, 3.0]
    lt = vp.candidate_grid(t, t, keep=lambda a, b: a < b)
    assert lt.shape == (3, 2) and (lt[:, 0] < lt[:, 1]).all()
    assert vp.candidate_grid(t, t, keep=lambda a, b: False).shape == (0, 2)
    assert vp.candidate_grid is search.candidate_grid
    with pytest.raises(ValueError):
        vp.candidate_grid()


@pytest.mark.parametrize("weighted", [False, True])
def test_numpy_mirror_ranks_like_a_plain_lstsq_loop(weighted):
    d = sc.base_data(37)
    mdl = sc.double_exp_model(d["x"])
    cand = sc.base_candidates()
    w = d["w"] if weighted else None
    cost, y2 = sc.base_costs(37, weighted)
    index, scores = search.rank_candidates(lambda a: sc.columns(mdl, d["x"], a), cand, d["Y"], w)
    assert index.dtype == np.int32 and scores.shape == cost.shape
    sc.check_fp64(index, None, cost, y2, 3, 37, 0.0)
    # a score is |y_w|^2 - 2 cost, to the bound the device's ranking is held to
    assert (np.abs(0.5 * (y2[:, None] - scores) - cost) <= sc.score_bound(3, 37, y2)[:, None]).all()
    # the rank-deficient candidate (2, 2) has one direction dropped, not a NaN
    Q = search.orthonormal_basis(sc.columns(mdl, d["x"], cand[-1]))
    assert np.isfinite(Q).all() and (np.abs(Q).sum(0) == 0).sum() == 1


def test_numpy_mirror_non_finite_candidates_and_right_hand_sides():
    d = sc.base_data(37)
    mdl = sc.double_exp_model(d["x"])
    basis_at = lambda a: sc.columns(mdl, d["x"], a)  # noqa: E731
    cand = np.vstack([[[np.nan, 4.0]], sc.base_candidates()])
    index, scores = search.rank_candidates(basis_at, cand, d["Y"])
    ref, _ = search.rank_candidates(basis_at, cand[1:], d["Y"])
    assert np.isneginf(scores[:, 0]).all() and np.array_equal(index, ref + 1)
    none, _ = search.rank_candidates(basis_at, cand[:1], d["Y"])
    assert (none == -1).all()
    # S right-hand sides: the scores add
    Y3 = np.stack([d["Y"], 0.5 * d["Y"][::-1], d["Y"] + 0.1], 1)
    _i, s3 = search.rank_candidates(basis_at, cand[1:], Y3)
    parts = sum(search.rank_candidates(basis_at, cand[1:], Y3[:, s])[1] for s in range(3))
    assert np.allclose(s3, parts, rtol=1e-13, atol=0)
