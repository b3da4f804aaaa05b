"""CPU tier of the per-kernel-set tests of the global-fit path (several right-hand sides): the case table of
tests/mrhs_cases.py against the registry, against find_kernels' rule for S > 1 and against the launchers' rules, the grids
against the library's criterion of a uniform grid, the conditions on the inputs that let the GPU tier compare EVERY problem,
and the oracle's Jacobian for S > 1 against a second witness.  No GPU: vp_debug_registry_entry and
vp_debug_registry_has_global only read the table of registered sets."""
import ctypes as C

import numpy as np
import pytest

import fit_cases as FC
import mrhs_cases as MC
import stats_cases as SC
from varpro_amd import _lib

ALL = MC.CASES
IDS = MC.IDS
# cond(W Phi) at the evaluation point: tests/test_fit_cases_host.py holds its fp64 cases to kappa_s <= 1e4, the range in which
# the numpy restatement (QR) and the oracle (SVD) agree to 1e-9 and the device holds 1e-10 with margin (largest ratio there
# 0.005); the same cap here, on the unscaled W Phi the factor kernel sees
COND_PHI_CAP = 1e4
# the column-scaled cond(J) up to which test_mrhs_gram_based_lm_step_conditioning_sweep holds the Gram-based step to 1e-9
COND_J_CAP = 1e3


def _global_sets():
    return set(_lib.registry_global_sets())


def test_case_ids_are_unique():
    assert len(set(IDS)) == len(IDS)


def test_registry_global_query():
    lib = _lib.load()
    n = len(_lib.registry_entries())
    assert lib.vp_debug_registry_has_global(n) == _lib.VP_ERR_INVALID
    assert lib.vp_debug_registry_has_global(-1) == _lib.VP_ERR_INVALID
    assert lib.vp_debug_registry_has_global(0) in (0, 1)
    # vp_debug_registry_entry returns what it did: 1 / 0 by the single-right-hand-side kernels alone
    rec = (C.c_int32 * 8)()
    assert all(lib.vp_debug_registry_entry(i, rec) in (0, 1) for i in range(n))
    sets = _lib.registry_global_sets()
    assert len(sets) == len(set(sets)) == 52
    # the three sets that serve several right-hand sides only
    only = {r for r, single in _lib.registry_entries() if not single}
    assert only == {SC.me_set(SC.F64, 2, 1, 32), SC.me_set(SC.F64, 3, 1, 32), SC.me_set(SC.F32, 2, 1, 32)} and only <= set(sets)
    # no multi-wave and no length-agnostic set among them
    assert all(r[6] == 1 and not r[7] for r in sets)


def test_every_registered_set_with_global_kernels_has_its_classes():
    registered = _global_sets()
    named = {gc.case.set for gc in ALL}
    missing = sorted(registered - named)
    assert not missing, "sets with multiple-right-hand-side kernels that no case names: %s" % [SC.set_name(r) for r in missing]
    unknown = sorted(named - registered)
    assert not unknown, "cases name sets that are not registered with such kernels: %s" % [SC.set_name(r) for r in unknown]
    by_set = {}
    for gc in ALL:
        by_set.setdefault(gc.case.set, []).append(gc.cls)
    for rec in sorted(registered):
        n, p, size = MC.set_columns(rec)
        R = rec[5]
        spills = (n + 1 + p) * R * (size // 4) > 400
        want = ["A", "B"] + (["C"] if R % 8 == 0 and not spills else [])
        assert sorted(c for c in by_set[rec] if c != "P") == want, (SC.set_name(rec), by_set[rec])
    # the one R % 8 == 0 set without a one-wave form, and the number of sets class C reaches
    assert [SC.set_name(r) for r in registered if r[5] % 8 == 0 and MC.one_wave_spills(r)] == ["me3o-f64-R32W1"]
    assert sum(gc.cls == "C" for gc in ALL) == 24
    # class P: one small and one R = 16 set of each family and dtype
    P = sorted((gc.case.set[0], gc.case.set[1], gc.case.set[5]) for gc in ALL if gc.cls == "P")
    assert P == sorted((dt, fam, R) for dt, fam in ((SC.F64, 1), (SC.F32, 1), (SC.F64, 2)) for R in (2, 16))


def _find_kernels(dtype, key, m, rt_key=None):
    """find_kernels (vp_api.hip) for S > 1 and unit or LDS-fitting weights: the smallest capacity wins; among equal
    capacities the set with multiple-right-hand-side kernels, then the fewest waves; a multi-exponential shape without a
    resident set of its own tries the run-time-descriptor sets of its (n, q, p)"""
    entries, glob = [r for r, _s in _lib.registry_entries()], _global_sets()
    best = None
    for k in [key] + ([rt_key] if rt_key else []):
        if best is not None and not best[7]:
            break
        for e in entries:
            if e[0] != dtype or e[1:5] != k or 64 * e[5] * e[6] < m:
                continue

            def better(x, y):
                if x[5] * x[6] != y[5] * y[6]:
                    return x[5] * x[6] < y[5] * y[6]
                if (x in glob) != (y in glob):
                    return x in glob
                return x[6] < y[6]
            if best is None or better(e, best):
                best = e
    return best


@pytest.mark.parametrize("gc", ALL, ids=IDS)
def test_case_sizes_select_their_set_and_the_records_follow_the_launchers_rules(gc):
    c = gc.case
    dtype, fam, a, b, cc, R, W, gen = c.set
    assert W == 1 and not gen and c.m <= 64 * R
    n, q = len(SC.SHAPES[c.shape].kinds), len(SC.SHAPES[c.shape].truth)
    rt_key = (_lib.FAMILY_RT, n, q, q) if fam == _lib.FAMILY_MULTIEXP else None
    assert _find_kernels(dtype, c.set[1:5], c.m, rt_key) == c.set
    # the classes are what the table says they are
    S, B = {"A": (3, 5), "B": (9, 5), "C": (2, 1025), "P": (3, 5)}[gc.cls]
    assert (gc.S, gc.B) == (S, B)
    if gc.cls == "A":
        assert c.m == 64 * R and c.uniform and c.weights is None and c.grid == "shared"
    elif gc.cls == "B":
        assert c.m == 64 * R - 1 and not c.uniform and c.weights == "shared" and c.grid == "shared"
    elif gc.cls == "C":
        assert R % 8 == 0 and c.m % 2 == 0 and c.uniform and c.weights is None and c.grid == "shared"
        assert _find_kernels(dtype, c.set[1:5], c.m - 2, rt_key) != c.set  # (the smallest even m of the set)
    else:
        assert c.weights == "per" and c.grid == "per"
    # the records, from the rules written out here a second time: B <= 1024, R % 8, the spill expression, vec, mrhs_gx
    size = 2 if dtype == SC.F64 else 1
    ncol, npair = (a + b, a) if fam == _lib.FAMILY_MULTIEXP else (a, cc)
    spills = (ncol + 1 + npair) * R * size > 400
    w = 4 if R % 8 == 0 and (B <= 1024 or spills) else 1
    coop, vec = dtype == SC.F64 and R == 32, c.m % 2 == 0
    gx = (S + 7) // 8
    assert gx == {3: 1, 9: 2, 2: 1}[S]
    assert MC.record(gc) == (0,) * 8
    assert MC.record(gc, evaluated=(True, True)) == (w, 0, 0, 3 if coop and vec else 1, 0, gx, 0, 0)
    assert MC.record(gc, evaluated=(True, False)) == (w, 0, 0, 4 if coop and vec else 1, 0, gx, 0, 0)
    assert MC.record(gc, evaluated=(False, False)) == (w, 0, 0, 1, 0, gx, 0, 0)
    assert MC.record(gc, fitted=True) == (0, w, 2 if coop and vec else 1, 0, gx, 0, 0, 0)
    assert MC.record(gc, evaluated=(True, True), fitted=True) == (w, w, 2 if coop and vec else 1, 3 if coop and vec else 1, gx, gx, 0, 0)
    if gc.cls == "C":
        assert w == 1
    elif R % 8 == 0:
        assert w == 4
    if gc.cls == "B":
        assert gx == 2 and S % 8 == 1  # two streaming workgroups, the second holding one column
    if coop:
        assert (MC.record(gc, fitted=True)[2] == MC.COOP_DMA) == (gc.cls in ("A", "C"))


def test_the_table_reaches_every_kernel_template_in_both_dtypes():
    """factor and step kernels in their one-wave and four-wave forms in fp64 and fp32, the streaming kernel in both modes, the
    cooperative kernels on each of the three fp64 R = 32 sets"""
    seen = set()
    for gc in ALL:
        rec = MC.record(gc, evaluated=(True, True), fitted=True)
        seen.add((gc.case.dtype, "waves", rec[0]))
        seen.add((gc.case.dtype, "fit", rec[2]))
        seen.add((gc.case.dtype, "eval", rec[3]))
    for dt in (SC.F64, SC.F32):
        assert {(dt, "waves", 1), (dt, "waves", 4), (dt, "fit", MC.STREAM), (dt, "eval", MC.STREAM)} <= seen
    assert {(SC.F64, "fit", MC.COOP_DMA), (SC.F64, "eval", MC.COOP_OUT_J)} <= seen
    coop = sorted(SC.set_name(gc.case.set) for gc in ALL if gc.cls == "A" and MC.is_coop(gc.case.set))
    assert coop == ["me1o-f64-R32W1", "me2o-f64-R32W1", "me3o-f64-R32W1"]
    assert {gc.case.set for gc in ALL if gc.case.dtype == SC.F32} == {SC.me_set(SC.F32, 2, 1, R) for R in (2, 8, 16, 32)} | {SC.me_set(SC.F32, 5, 1, 2)}


@pytest.mark.parametrize("gc", ALL, ids=IDS)
def test_grids_are_uniform_or_not_by_the_librarys_criterion(gc):
    c = gc.case
    assert MC.handle_grid_uniform(gc) == (c.uniform and c.grid == "shared") == (gc.cls in ("A", "C"))


def test_noise_is_1e_3_but_for_the_small_cases_of_five_exponentials():
    quiet = [gc for gc in ALL if gc.case.noise != SC.NOISE]
    assert [(gc.cls, gc.case.shape, gc.case.m, gc.case.noise) for gc in quiet] == [("A", "me5o", 128, 1e-5), ("B", "me5o", 127, 1e-5)]


@pytest.mark.parametrize("gc", ALL, ids=IDS)
def test_the_evaluation_point_is_well_conditioned_and_a_second_witness_agrees(gc):
    """cond(W Phi) under the cap; C, r, cost and J of the numpy restatement (QR, column by column) against the oracle (SVD,
    all columns at once) to 1e-9; fp32 cases: finite bounds well under 1"""
    c, d = gc.case, MC.case_data(gc)
    assert (MC.oracle_evaluate(gc)["status"] == 0).all()
    for b, e in enumerate(MC.numpy_evaluate_errors(gc, np.float64)):
        assert e["kappa"] <= COND_PHI_CAP, (b, e["kappa"])
        for k in MC.EVAL_KEYS:
            assert e[k] <= 1e-9, (b, k, e)
    assert np.abs(d["alpha"] / np.asarray(SC.SHAPES[c.shape].truth) - 1.0).max() <= 0.04 + 1e-6
    if c.dtype == SC.F32:
        bounds = MC.fp32_eval_bounds(gc)
        print(MC.gcase_id(gc), "fp32 bounds", bounds)
        assert all(np.isfinite(v) and v < 0.05 for v in bounds.values()), bounds


@pytest.mark.parametrize("gc", ALL, ids=IDS)
def test_the_oracles_own_global_fit_succeeds_and_the_jacobian_is_well_conditioned(gc):
    """What lets the GPU tier compare every problem of every fit: the oracle's own fit of each distinct problem succeeds, and the
    column-scaled cond(J) of the stacked (S m) x q Jacobian is <= 1e3 at the start point and at the oracle's minimum"""
    c, d, ref = gc.case, MC.case_data(gc), MC.oracle_fit(gc)
    q = len(SC.SHAPES[c.shape].truth)
    assert np.abs(d["guess"] / np.asarray(SC.SHAPES[c.shape].truth) - 1.0).max() <= 0.05 + 1e-6
    assert (ref["termination"] > 0).all(), ref["termination"]
    for b in range(MC.NB):
        k0, k1 = MC.scaled_cond_J(gc, b, d["guess"][b]), MC.scaled_cond_J(gc, b, ref["alpha"][b])
        print("%s problem %d: %d evaluations  cond(J) start %.3e  minimum %.3e" % (MC.gcase_id(gc), b, ref["n_evals"][b], k0, k1))
        assert k0 <= COND_J_CAP and k1 <= COND_J_CAP, (b, k0, k1)
        # the trace is long enough for the trajectory comparison: three rows above 1e-6 of the first cost
        tr = ref["trace"][b]
        assert (tr[:6, q] >= 1e-6 * tr[0, q]).sum() >= 3, tr[:, q]
    if c.dtype == SC.F32:
        ex = MC.oracle_fit_f32_excess(gc)
        print(MC.gcase_id(gc), "fp32 reference excess", ex, "ftol", FC.device_ftol32())
        assert np.isfinite(ex).all() and (ex < 1e-2).all(), ex


ONE_PER_SHAPE = list({gc.case.shape: gc for gc in ALL if gc.cls == "B"}.values())  # (class B: weights, nine columns)


@pytest.mark.parametrize("gc", ONE_PER_SHAPE, ids=[MC.gcase_id(gc) for gc in ONE_PER_SHAPE])
def test_the_oracles_stacked_jacobian_against_a_second_witness(gc):
    """-P_perp (W D_k c_s), column s after column s, from a QR of W Phi in numpy: 1e-9 of max |J_k|"""
    d, ref = MC.case_data(gc), MC.oracle_evaluate(gc)
    assert len(ONE_PER_SHAPE) == len({g.case.shape for g in ALL})
    for b in range(MC.NB):
        x, Y, w = MC.problem_inputs(d, b)
        J = MC.numpy_jacobian(d["model"], x, Y, w, d["alpha"][b].astype(np.float64))
        assert J.shape == ref["J"][b].shape == (ref["J"].shape[1], gc.S * gc.case.m)
        for k in range(J.shape[0]):
            assert np.abs(J[k] - ref["J"][b, k]).max() <= 1e-9 * np.abs(ref["J"][b, k]).max(), (b, k)
