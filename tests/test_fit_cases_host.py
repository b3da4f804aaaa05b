"""CPU tier of the per-kernel-set tests of the evaluation and fit kernels: the case table of tests/fit_cases.py against the
registry and against launch_fit's selection, the grids against the library's criterion of a uniform grid, the conditions on
the inputs that let the GPU tier compare EVERY problem, and the oracle's Jacobian against a second witness.  No GPU.
The whole file runs in about 8 s (848 tests), so class D stays for the run-time-descriptor sets too."""
import numpy as np
import pytest

import fit_cases as FC
import stats_cases as SC
from varpro_amd import _lib

ALL = FC.FIT_CASES
IDS = FC.IDS


def _single_rhs_sets():
    return {rec for rec, single in _lib.registry_entries() if single}


def test_case_ids_are_unique():
    assert len(set(IDS)) == len(IDS)


def test_noise_is_1e_3_but_for_the_four_small_cases_of_five_exponentials():
    quiet = [fc for fc in ALL if fc.case.noise != SC.NOISE]
    assert len(quiet) == 4 and all(fc.case.noise == 1e-5 and fc.case.shape == "me5o" and fc.case.m <= 130 for fc in quiet)
    assert {fc.cls for fc in quiet} == {"A", "B", "C"}


def test_every_registered_set_with_a_fit_kernel_has_a_case_of_each_class():
    reachable = _single_rhs_sets()  # (every set that carries an evaluation kernel carries a fit kernel: vp_inst.hpp)
    generic = {SC.gen_set(SC.F64), SC.gen_set(SC.F32)}  # (not in the table: vp_batch_create's fallback)
    named = {fc.case.set for fc in ALL}
    assert generic <= named
    missing = sorted(reachable - named)
    assert not missing, "sets no fit case names: %s" % [SC.set_name(r) for r in missing]
    unknown = sorted(named - reachable - generic)
    assert not unknown, "fit cases name sets that are not registered: %s" % [SC.set_name(r) for r in unknown]
    by_set = {}
    for fc in ALL:
        by_set.setdefault(fc.case.set, set()).add(fc.cls)
    for rec in sorted(reachable):
        dtype, _fam, _a, _b, _c, R, W, gen = rec
        if gen:
            assert by_set[rec] == {"L"}, SC.set_name(rec)
            continue
        below = max([64 * r[5] * r[6] for r in reachable if r[:5] == rec[:5] and r[5] * r[6] < R * W], default=0)
        want = {"A", "B", "C"} | ({"D"} if 64 * (R - 2) * W > below else set())
        assert want <= by_set[rec] <= want | {"P"}, (SC.set_name(rec), by_set[rec])


def test_the_slot_kernel_sets_are_the_ones_that_end_in_a_constant_column():
    # the multi-exponential sets with an offset, but for the fp32 Gram set and for me1o at R 32, whose slots do not fit the LDS:
    # me1o at R 2 8 16 24, me2o at 2 4 8 12 16 20, me3o at 2 8 16 20 and four waves of 8 in fp64; me2o at 2 8 16 and me5o at 2
    # in fp32
    launcher = {r for r in _single_rhs_sets() if FC.slot_launcher(r)}
    slots = sorted(SC.set_name(r) for r in launcher if FC.has_slot_kernel(r))
    assert len(launcher) == 20 and len(slots) == 19, slots
    # by the LDS rule, not by name: the one set without room (the GPU tier asserts that "slots" reports the wave kernel there,
    # and the slot kernel everywhere else -- a rule that misjudged a set would fail one of the two)
    assert [SC.set_name(r) for r in launcher if not FC.slots_fit_lds(r)] == ["me1o-f64-R32W1"]
    # EVERY set with the launcher is in the slot tests, the one without room included
    assert {fc.case.set for fc in ALL if fc.slots is not None} == launcher
    for r in launcher:
        classes = {fc.cls for fc in ALL if fc.case.set == r and fc.slots is not None and fc.case.weights is None}
        assert {"A", "B"} <= classes, SC.set_name(r)
    for fc in FC.REFILL_CASES:
        assert fc.slots == (FC.SLOTS, 1, 0, 0)
    assert len(FC.REFILL_CASES) == 2


@pytest.mark.parametrize("fc", ALL, ids=IDS)
def test_case_sizes_follow_the_selection_rule_and_lie_in_their_padding_class(fc):
    c = fc.case
    dtype, fam, a, b, cc, R, W, gen = c.set
    if fam == _lib.FAMILY_GENERIC:
        assert fc.wave == (FC.GENERIC, -1, int(c.weights is not None), 0) and fc.slots is None
        return
    # find_kernels: the smallest 64 R W >= m among the sets of the key that a single-RHS handle can take; a multi-exponential
    # shape also runs on the run-time-descriptor set of its (n, q, p), which a length-agnostic set loses against
    n, q = len(SC.SHAPES[c.shape].kinds), len(SC.SHAPES[c.shape].truth)
    keys = [c.set[:5]] + ([(dtype, _lib.FAMILY_RT, n, q, q)] if fam == _lib.FAMILY_MULTIEXP else [])
    resident = [r for r in _single_rhs_sets() if r[:5] in keys and not r[7]]
    if gen:
        assert R == SC.BLK_R and fc.wave == (FC.BLOCK, -1, int(c.weights is not None), 0) and fc.slots is None
        if not c.stream:
            cap = max([64 * r[5] * r[6] for r in resident], default=0)
            assert c.m > cap and (cap == 0 or c.m == cap + 1), "%d rows: the largest resident set holds %d" % (c.m, cap)
        else:
            assert c.m % (64 * 8) != 0  # (block_rows of six fp64 columns: 8 rows per lane)
        return
    assert c.m <= 64 * R * W
    for r in resident:
        if r[:5] == c.set[:5] and r[5] * r[6] < R * W:
            assert 64 * r[5] * r[6] < c.m, "%s covers m = %d" % (SC.set_name(r), c.m)
    weighted = c.weights is not None
    if FC.is_gram(c.set):
        assert fc.wave[0] == FC.GRAM and fc.slots is None
        return
    assert fc.wave == (FC.WAVE, 0 if weighted else FC.padding_class(c.m, R, W), int(weighted), 0)
    want_cls = {"A": 1, "B": 2 if R > 2 else 0, "C": 0, "D": 0}
    if fc.cls in want_cls:
        assert fc.wave[1] == want_cls[fc.cls]
        assert (c.m % 2 == 1) == (fc.cls == "B") and weighted == (fc.cls == "C")
        if fc.cls == "D":
            assert R > 2 and c.m <= 64 * (R - 2) * W
    if FC.slot_launcher(c.set):
        # outside the slot kernel's coverage, or no room in the LDS: launch_fit2 hands over to launch_fit
        if weighted or c.grid == "per" or not FC.slots_fit_lds(c.set):
            assert fc.slots == fc.wave
        else:
            assert fc.slots == (FC.SLOTS, fc.wave[1], 0, 0)
    else:
        assert fc.slots is None


@pytest.mark.parametrize("fc", ALL, ids=IDS)
def test_grids_are_uniform_or_not_by_the_librarys_criterion(fc):
    """grid_check_kernel: dt = (t[m-1] - t[0]) / (m - 1) finite and non-zero and |t[i] - fma(i, dt, t[0])| <= 4 eps |t[i] - t[0]|
    for every i, eps that of the handle's dtype, evaluated in fp64 on the handle's own grid"""
    c = fc.case
    assert FC.handle_grid_uniform(c) == (c.uniform and c.grid == "shared")
    if fc.cls != "P":
        assert c.uniform == (fc.cls in ("A", "C", "G") or (fc.cls == "L" and not c.stream))


@pytest.mark.parametrize("fc", ALL, ids=IDS)
def test_the_oracles_own_fit_succeeds_and_its_minimum_is_well_conditioned(fc):
    """The condition that lets the GPU tier compare every problem of every fit: from fit_guess the oracle's own fit of each
    problem succeeds, and at its minimum kappa_s <= 1e4 and cond(H)^2 eps_longdouble <= 1e-10.  (Five exponentials + offset
    on <= 130 rows meet it at a noise of 1e-5 only: fit_cases._inputs has the figures.)"""
    c = fc.case
    d, ref = SC.case_data(c), FC.oracle_fit(c)
    assert np.abs(SC.fit_guess(c) / np.asarray(SC.SHAPES[c.shape].truth) - 1.0).max() <= 0.05 + 1e-6
    assert (ref["termination"] > 0).all(), ref["termination"]
    for b in range(SC.B):
        x, y, w = SC.problem_inputs(d, b)
        at = SC.reference_at(d["model"], x, y, w, ref["alpha"][b], SC.F64)  # (the conditioning: no fp32 restatement needed)
        print("%s problem %d: %d evaluations  kappa_s %.3e  cond(H) %.3e" % (FC.fit_case_id(fc), b, ref["n_evals"][b],
                                                                          at["kappa_s"], at["cond_H"]))
        assert at["kappa_s"] <= 1e4, (b, at["kappa_s"])
        assert at["cond_H"] ** 2 * SC.EPS_LONGDOUBLE <= 1e-10, (b, at["cond_H"])
        # the fit's trace is long enough for the trajectory comparison: three rows above 1e-6 of the first cost
        tr, q = ref["trace"][b], len(SC.SHAPES[c.shape].truth)
        assert (tr[:6, q] >= 1e-6 * tr[0, q]).sum() >= 3, tr[:, q]


@pytest.mark.parametrize("fc", ALL, ids=IDS)
def test_numpy_restatement_of_the_evaluation_agrees_with_the_oracle(fc):
    """C, r, the cost and the Kaufman Jacobian J_k = -P_perp (W D_k c) from a QR of W Phi in fp64 against the oracle (SVD):
    1e-9 of max |J_k| and of the other quantities' scales"""
    c = fc.case
    assert (FC.oracle_evaluate(c)["status"] == 0).all()
    for b, e in enumerate(FC.numpy_evaluate_errors(c, np.float64)):
        for k in FC.EVAL_KEYS:
            assert e[k] <= 1e-9, (b, k, e)
    if c.dtype == SC.F32:
        bounds = FC.fp32_eval_bounds(c)
        print(FC.fit_case_id(fc), "fp32 bounds", bounds)
        assert all(np.isfinite(v) and v < 0.05 for v in bounds.values()), bounds
