"""CPU tier of the per-kernel-set statistics tests: the case table of tests/stats_cases.py against the registry, its two
references against each other, and the conditioning of its inputs.  No GPU: the library loads without one and
vp_debug_registry_entry only reads the table of registered sets."""
import numpy as np
import pytest

import stats_cases as SC
from oracle import oracle as O
from varpro_amd import _lib

ALL = SC.CASES + SC.PER_PROBLEM_CASES + SC.DOF_EDGE_CASES + SC.FIT_CASES
IDS = [SC.case_id(c) for c in ALL]


def test_case_ids_are_unique():
    assert len(set(IDS)) == len(IDS)


def test_every_registered_single_rhs_set_is_named_by_a_case():
    entries = _lib.registry_entries()
    assert len(entries) > 50
    assert len(set(rec for rec, _ in entries)) == len(entries), "two registrations with the same key"
    reachable = {rec for rec, single_rhs in entries if single_rhs}
    named = {c.set for c in ALL}
    generic = {SC.gen_set(SC.F64), SC.gen_set(SC.F32)}  # (not in the table: vp_batch_create's fallback)
    assert generic <= named
    missing = sorted(reachable - named)
    assert not missing, "sets no case names: %s" % [SC.set_name(r) for r in missing]
    unknown = sorted(named - reachable - generic)
    assert not unknown, "cases name sets that are not registered: %s" % [SC.set_name(r) for r in unknown]


def test_registry_query_ends_with_invalid():
    import ctypes as C
    rec = (C.c_int32 * 8)()
    lib = _lib.load()
    n = len(_lib.registry_entries())
    assert lib.vp_debug_registry_entry(n, rec) == _lib.VP_ERR_INVALID
    assert lib.vp_debug_registry_entry(-1, rec) == _lib.VP_ERR_INVALID
    assert lib.vp_debug_registry_entry(0, rec) in (0, 1)


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_case_sizes_follow_the_selection_rule(c):
    """a case's m lies in its set: m <= 64 R W, and beyond every smaller registered set of the same key that a
    single-right-hand-side handle can take (find_kernels: the smallest 64 R W >= m)"""
    dtype, fam, a, b, cc, R, W, _gen = c.set
    if fam == _lib.FAMILY_GENERIC:
        return
    assert c.m <= 64 * R * W
    if c.stream:
        assert R == SC.BLK_R
        return
    same_key = [rec for rec, single in _lib.registry_entries() if single and rec[:5] == c.set[:5]]
    for rec in same_key:
        if rec[5] * rec[6] < R * W:
            assert 64 * rec[5] * rec[6] < c.m, "%s covers m = %d" % (SC.set_name(rec), c.m)


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_numpy_restatement_agrees_with_the_oracle_and_inputs_are_well_conditioned(c):
    refs = SC.reference(c)
    k = len(SC.SHAPES[c.shape].kinds) + len(SC.SHAPES[c.shape].truth)
    for b, ref in enumerate(refs):
        assert ref["stats"] is not None and ref["stats"]["dof"] == c.m - k
        print("%s problem %d: kappa_s %.3e  cond(H) %.3e  e_np64 %s%s" % (SC.case_id(c), b, ref["kappa_s"], ref["cond_H"],
              ref["e_np64"], "  e_np32 %s" % ref["e_np32"] if c.dtype == SC.F32 else ""))
        # the oracle is not the only witness
        for key in ("cov", "sigma", "chi2"):
            assert ref["e_np64"][key] <= 1e-9, (b, key, ref["e_np64"])
        # a condition on the INPUTS: the oracle solves the normal equations in long double, so its own error
        # cond(H)^2 eps_longdouble stays two orders inside the fp64 tolerance 1e-8
        assert ref["kappa_s"] <= 1e4, (b, ref["kappa_s"])
        assert ref["cond_H"] ** 2 * SC.EPS_LONGDOUBLE <= 1e-10, (b, ref["cond_H"])
        if c.dtype == SC.F32:  # the fp32 tolerances are finite and stay tolerances
            assert all(np.isfinite(v) and v < 0.05 for v in ref["tol"].values()), ref["tol"]


@pytest.mark.parametrize("c", SC.FIT_CASES, ids=[SC.case_id(c) for c in SC.FIT_CASES])
def test_the_oracles_own_fits_of_the_fit_cases_all_succeed(c):
    d = SC.case_data(c)
    g = SC.fit_guess(c)
    assert np.abs(g / np.asarray(SC.SHAPES[c.shape].truth) - 1.0).max() <= 0.05 + 1e-6
    for b in range(SC.B):
        x, y, w = SC.problem_inputs(d, b)
        p = O.Problem(d["model"], x, y, w=w)
        p.set_params(g[b].astype(np.float64))
        assert p.fit().termination > 0, b
        ref = SC.reference_at(d["model"], x, y, w, p.params(), c.dtype)
        assert ref["kappa_s"] <= 1e4 and ref["cond_H"] ** 2 * SC.EPS_LONGDOUBLE <= 1e-10, (b, ref["kappa_s"], ref["cond_H"])


@pytest.mark.parametrize("shape,dtype,kset", SC.DOF_EDGE_SETS)
@pytest.mark.parametrize("dof", [0, -1])
def test_the_oracle_reports_underdetermined_statistics(shape, dtype, kset, dof):
    c = SC.dof_edge_case(shape, dtype, kset, dof)
    for ref in SC.reference(c):
        assert ref["stats"] is None and ref["best_fit"] is not None
