"""The slot kernel with its issue-priority sections (VP_FIT2_CHAIN_PRIO, vp_fit2.hpp) and with the rare-branch marks of the
two-column Jacobian factorisation (VP_JAC_Q2_NOCOPY, vp_fit.hpp) against the wave kernel ON THE SAME HANDLE, bit for bit: the
priority of a wave only picks among ready waves and the marks only move register copies, so parameters, termination codes,
evaluation counts and objectives must not change by one bit -- the contract of tests/test_gpu_slot_kernel.py, restated for
the code paths the two switches touch: the three padding variants of the 16-rows-per-lane set (m = 1024, 1000 / 900, 880), the
queue, the refill and the lone tail (B = 600), BOTH pivot orders of the factorisation, and multi-wave groups (W = 4): the fp32 five-exponential shape, whose fit is the Gram
kernel's under every selection, and the fp64 triple exponential, which has a four-wave slot kernel."""
import functools

import numpy as np
import pytest

import fit_cases as FC
import varpro_amd as vp
from models import double_exp_builder_model
from oracle import oracle as O
from varpro_amd import synth

pytestmark = pytest.mark.gpu

WAVE, SLOTS = 1, 2  # vp_debug_last_fit: the kernel the launcher issued
B = 600
# launch_fit2's instantiation by length at 16 rows per lane: 1 = m == 64 R, 2 = padding in the last register pair only (m > 896),
# 0 = general.  (1024, 1000 and 900 are two of the three -- 900 > 896 --, so 880 is here for the third)
PADDING_CLASS = {1024: 1, 1000: 2, 900: 2, 880: 0}
LENGTHS = sorted(PADDING_CLASS, reverse=True)


@functools.lru_cache(maxsize=None)
def _batch(m):
    """B double exponential + offset problems (noise 1e-3) in which every second problem has its two exponentials exchanged:
    the data do not know which exponential is `first`, so exchanging the amplitudes and the decay times of the truth is
    exchanging the two initial guesses -- and with them the two Kaufman Jacobian columns, i.e. the pivot order.  Returns the
    batch and the pivot column of the first factorisation per problem, from the ORACLE's Jacobian at the initial guess
    (MINPACK qrfac takes the column of largest norm first)."""
    d = synth.double_exp_batch(B, m=m, noise=1e-3)
    guess = d["tau_guess"].copy()
    guess[1::2] = guess[1::2, ::-1]
    mdl = double_exp_builder_model(d["x"], guess[0])
    ev = O.evaluate_batch(mdl, d["x"], d["Y"], guess, n_threads=4)
    assert (ev["status"] == 0).all()
    norms = np.linalg.norm(ev["J"], axis=2)  # [B, 2]
    first_pivot = (norms[:, 1] > norms[:, 0]).astype(int)
    for a in (d["Y"], guess, first_pivot):
        a.setflags(write=False)
    return d["x"], d["Y"], guess, mdl, first_pivot


def _fit(bp, kernel, guess, expect):
    bp.set_fit_kernel(kernel)
    a, c, r = bp.fit(guess)
    assert bp.last_fit_kernel()[:len(expect)] == expect, bp.last_fit_kernel()
    return a, r


def _same(wave, slots):
    (a0, r0), (a1, r1) = wave, slots
    assert np.array_equal(r0["termination"], r1["termination"])
    assert np.array_equal(r0["n_evals"], r1["n_evals"])
    assert np.array_equal(r0["objective"], r1["objective"], equal_nan=True)
    assert np.array_equal(a0, a1, equal_nan=True)


@pytest.mark.parametrize("m", LENGTHS)
def test_both_pivot_orders_occur(m):
    # (host arithmetic only, but part of this file's premise: without it the untouched order is all the GPU test would see)
    first_pivot = _batch(m)[4]
    share = first_pivot.mean()
    print("m = %d: pivot column 1 first in %.1f %% of the problems" % (m, 100 * share))
    assert 0.25 <= share <= 0.75, share


@pytest.mark.parametrize("m", LENGTHS)
def test_slot_kernel_with_priority_sections_equals_wave_kernel(m):
    x, Y, guess, mdl, first_pivot = _batch(m)
    assert 0.25 <= first_pivot.mean() <= 0.75
    bp = vp.BatchProblem(mdl, Y, x=x)
    wave = _fit(bp, "wave", guess, (WAVE,))
    slots = _fit(bp, "slots", guess, (SLOTS, PADDING_CLASS[m]))
    bp.close()
    _same(wave, slots)
    assert (wave[1]["termination"] > 0).mean() > 0.9  # (the batch is one that fits: accepted steps, i.e. factorisations, happen)
    # the batch permuted: a problem's result does not depend on the wave, the slot or the moment it ran in
    perm = np.random.default_rng(11).permutation(B)
    bp = vp.BatchProblem(mdl, Y[perm], x=x)
    wave_p = _fit(bp, "wave", guess[perm], (WAVE,))
    slots_p = _fit(bp, "slots", guess[perm], (SLOTS, PADDING_CLASS[m]))
    bp.close()
    _same(wave_p, slots_p)
    _same((slots[0][perm], slots[1][perm]), slots_p)


def test_fp32_five_exponentials_four_waves_is_untouched():
    # fp32, five exponentials + offset, m = 4096, four waves per problem: every fit-kernel selection of this shape runs the
    # Gram kernel (vp_fitg.hpp; fit_cases.is_gram), which has a plain Grp -- the helpers are nothing there.  Asserted: that
    # kernel is what ran under either selection, and the two fits agree bit for bit
    taus = [0.5, 1.5, 3.0, 6.0, 12.0]
    d = synth.multi_exp_batch(64, 5, 4096, taus, noise=1e-3, spread=0.1, guess_spread=0.05, dtype=np.float32)
    mdl = vp.multi_exponential_model(d["x"], d["tau_guess"][0], dtype=np.float32)
    bp = vp.BatchProblem(mdl, d["Y"], x=d["x"])
    wave = _fit(bp, "wave", d["tau_guess"], (FC.GRAM, -1))
    slots = _fit(bp, "slots", d["tau_guess"], (FC.GRAM, -1))
    bp.close()
    _same(wave, slots)


def test_multi_wave_slot_kernel_with_priority_sections_equals_wave_kernel():
    # the multi-wave group that DOES have a slot kernel: three exponentials + offset in fp64 on four waves (8 rows per lane,
    # m = 2048).  Its reductions go through LDS and workgroup barriers with the priority raised, its three-column factorisation
    # is the generic routine (no helpers).  The problems of tests/test_gpu_fit_sets.py's refill test, computed once for both
    (fc,) = [f for f in FC.REFILL_CASES if f.case.set[6] == 4]
    d = FC.refill_data(fc.case)
    bp = vp.BatchProblem(d["model"], d["Y"], x=d["x"])
    assert bp.kernel_set() == fc.case.set
    wave = _fit(bp, "wave", d["guess"], fc.wave)
    slots = _fit(bp, "slots", d["guess"], fc.slots)
    bp.close()
    assert fc.slots[0] == SLOTS
    assert (wave[1]["termination"] > 0).mean() > 0.9
    _same(wave, slots)
