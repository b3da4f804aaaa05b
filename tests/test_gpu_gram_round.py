"""The slot kernel's single reduction round for ||r||^2 and the Jacobian's Gram values (VP_FIT2_GRAM_ROUND, vp_fit2.hpp) against
the wave kernel ON THE SAME HANDLE, bit for bit.  fit_kernel keeps the two rounds -- ||r||^2 alone, then the accept decision, then
the Gram round inside jac_qrfac_scaled -- so parameters, termination codes, evaluation counts, objectives and the first eight
trace rows must not differ by one bit (the contract of tests/test_gpu_slot_kernel.py), here on the inputs where the merged round
could differ from the two:

  * a rank-deficient start: the linear solve takes truncated_solve and the range(Q) part e of the residual is not zero, where
    the two rounds multiply e by a cleared row of the derivative column and the one round multiplies two zeros;
  * evaluations that are not finite: the Gram values travel with a non-finite ||r||^2 and must go unused;
  * rejected trial steps: the Gram values were formed for nothing, and the next accepted step must not see them;
  * one and three exponentials (3 and 10 values in the round, other row masks), each on a slot set of its own;
  * the lone tail, which has its own call site.

Every shape is the smallest that reaches its path: more problems than one wave's slots, one batch per case."""
import numpy as np
import pytest

import varpro_amd as vp
from models import double_exp_builder_model
from oracle import oracle as O
from varpro_amd import synth

pytestmark = pytest.mark.gpu

WAVE, SLOTS = 1, 2  # vp_debug_last_fit: the kernel the launcher issued
USER = -1           # VP_TERM_USER: an evaluation that is not finite
TRACE_ROWS = 8


def _fit(bp, kernel, guess, expect):
    bp.set_fit_kernel(kernel)
    a, c, r, t = bp.fit_trace(guess, max_rows=TRACE_ROWS)
    assert bp.last_fit_kernel()[:len(expect)] == expect, bp.last_fit_kernel()
    return a, r, t


def _wave_and_slots(mdl, Y, x, guess, padding, epsilon=None):
    bp = vp.BatchProblem(mdl, Y, x=x, epsilon=epsilon)
    wave = _fit(bp, "wave", guess, (WAVE,))
    slots = _fit(bp, "slots", guess, (SLOTS, padding))
    bp.close()
    (a0, r0, t0), (a1, r1, t1) = wave, slots
    assert np.array_equal(r0["termination"], r1["termination"])
    assert np.array_equal(r0["n_evals"], r1["n_evals"])
    assert np.array_equal(r0["objective"], r1["objective"], equal_nan=True)
    assert np.array_equal(a0, a1, equal_nan=True)
    assert np.array_equal(t0, t1, equal_nan=True)
    return wave


# launch_fit2's variant by length at the double exponential's sets: 1024 fills 16 rows per lane, 1000 pads the last register pair,
# 300 is the general variant of the 8-rows-per-lane set
@pytest.mark.parametrize("epsilon", [None, 1e-6])
@pytest.mark.parametrize("gap", [0.0, 1e-9])
@pytest.mark.parametrize("m,padding", [(1024, 1), (1000, 2), (300, 0)])
def test_rank_deficient_start(m, padding, gap, epsilon):
    # both decay times equal, or 1e-9 apart: the two exponential columns coincide (sigma_min of Phi at the guess: 5e-18 .. 1e-14
    # and 5e-10 .. 3e-9).  With epsilon = 1e-6 every first evaluation is below the threshold and takes truncated_solve (e != 0);
    # with the default (machine epsilon) the equal columns mostly pass the rank test and solve an all but singular triangle
    d = synth.double_exp_batch(67, m=m, noise=1e-3)
    guess = d["tau_guess"].copy()
    guess[:, 1] = guess[:, 0] + gap
    mdl = double_exp_builder_model(d["x"], guess[0])
    if epsilon is not None:
        smin = [np.linalg.svd(O.eval_phi(mdl, d["x"], guess[b]).T, compute_uv=False)[-1] for b in range(0, 67, 11)]
        assert max(smin) < epsilon, smin  # (the truncated path IS what the first evaluation takes)
    _wave_and_slots(mdl, d["Y"], d["x"], guess, padding, epsilon)


def test_non_finite_evaluations():
    # every third problem starts at a decay time of 0.05, from where the first steps overshoot through zero -- exp(+x / |tau|)
    # overflows at a TRIAL point in some of them (asserted below); every third starts at -0.004 and overflows at once
    d = synth.double_exp_batch(35, m=1024, noise=1e-3)
    guess = d["tau_guess"].copy()
    guess[::3, 0] = 0.05
    guess[1::3, 0] = -0.004
    mdl = double_exp_builder_model(d["x"], guess[0])
    a, r, t = _wave_and_slots(mdl, d["Y"], d["x"], guess, 1)
    user = r["termination"] == USER
    print("non-finite at the start: %d, at a trial point: %d of 35" % ((user & (r["n_evals"] == 1)).sum(), (user & (r["n_evals"] > 1)).sum()))
    assert (user & (r["n_evals"] == 1)).any() and (user & (r["n_evals"] > 1)).any()
    assert (r["termination"] > 0).any()


def test_rejected_first_trial_steps():
    # guesses three times the true decay times: the first trial step is rejected (every one of the oracle's fits sampled) --
    # its Gram values go unused, and the old factor is re-used for the next step
    d = synth.double_exp_batch(129, m=1024, noise=1e-3)
    guess = 3.0 * d["tau_true"]
    mdl = double_exp_builder_model(d["x"], guess[0])
    a, r, t = _wave_and_slots(mdl, d["Y"], d["x"], guess, 1)
    ratio = t[:, 1:, 3]  # trace rows: [alpha_trial (2), ||r||, ratio, delta, par]; row 0 is the initial point (ratio NaN)
    rejected = (ratio < 1.0e-4).any(axis=1)
    print("problems with a rejected step in the first %d evaluations: %d of 129" % (TRACE_ROWS, rejected.sum()))
    assert rejected.any()
    assert (r["termination"] > 0).mean() > 0.9


# (decay times, m, rows per lane of the set): one exponential + offset at 8 and 16 rows per lane, three at 8
@pytest.mark.parametrize("taus,m", [((2.0,), 512), ((2.0,), 1024), ((1.0, 3.0, 9.0), 512)])
def test_one_and_three_exponentials(taus, m):
    d = synth.multi_exp_batch(45, len(taus), m, list(taus), noise=1e-3, spread=0.1, guess_spread=0.1)
    mdl = vp.multi_exponential_model(d["x"], d["tau_guess"][0])
    a, r, t = _wave_and_slots(mdl, d["Y"], d["x"], d["tau_guess"], 1)
    assert (r["termination"] > 0).mean() > 0.9  # (accepted steps, i.e. factorisations, happen)


def test_lone_tail():
    # 4 099 problems on 4 096 slots (256 CUs x 8 waves x 2): the queue is dry after three pops, and every wave ends with a single
    # fit left -- fit2_lone_tail finishes it
    d = synth.double_exp_batch(4099, m=1024, noise=1e-3)
    mdl = double_exp_builder_model(d["x"], d["tau_guess"][0])
    a, r, t = _wave_and_slots(mdl, d["Y"], d["x"], d["tau_guess"], 1)
    assert (r["termination"] > 0).mean() > 0.9
