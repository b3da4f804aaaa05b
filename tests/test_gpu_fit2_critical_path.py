"""The slot kernel's per-iteration critical path (vp_fit2.hpp: wave-uniform launch values in SGPRs, out-of-line functions with
internal linkage, the refill section skipped when no slot of the group finished) must not change a bit of any result: every
case forces the slot kernel and compares it with the one-wavefront-per-problem kernel -- same arithmetic per problem -- bit
for bit on parameters, reports and evaluation counts.

The batches are chosen around the refill section: more problems than the persistent grid holds (every slot is refilled several
times and the queue runs dry while waves are mid-fit), batches that leave slots empty from the start and go straight to the lone
tail, groups of four waves of the triple exponential (the skip is a branch every wave of a workgroup must take alike), the padded kernel variants, and
problems that are flagged and re-fitted by the wave that flagged them.

What these tests do NOT check: VP_FIT2_SKIP_REFILL (and VP_FIT2_LOCAL_CALLS) lost their A/B and are off in the shipped build, so
the "refill_skip" cases run the refill section in every iteration there -- they exercise the skip only in a build made with
-DVP_FIT2_SKIP_REFILL=1 (as the switch was measured; all cases passed on it).  In the shipped build they check the item that is
on (VP_FIT2_SCALARS) and the batches' shapes.  Nor can a test tell the slot kernel from a quiet fall-back to the wave kernel:
the C API has no hook for it; that the triple-exponential shapes launch fit2_kernel<..., W = 4> is a one-time record
(profiles/critical_path_w4_kernel_trace.json), not an assertion."""
import os
import subprocess
import sys

import numpy as np
import pytest

import contracts as K
import varpro_amd as vp
from oracle import oracle as O
from varpro_amd import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GS, NG = 2, 4  # fp64 double exponential at 16 rows per lane: slots per wave, one-wave groups per workgroup


def _grid_slots():
    """problems the persistent grid of the m = 1024 slot kernel holds at once: 2 workgroups per CU x NG waves x GS slots"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 2 * NG * GS


def _batch(B, m, grid="uniform", distinct=1024):
    """B double-exponential problems: `distinct` generated ones, repeated (a slot's result does not depend on its neighbours);
    grid "log": log-spaced abscissae -- not a uniform grid, so the kernel evaluates every row's exponential (per-row branch)"""
    d = synth.double_exp_batch(min(B, distinct), m=m, noise=1e-3)
    x, Y, g = d["x"], d["Y"], d["tau_guess"]
    if grid == "log":
        x = np.geomspace(0.01, 12.5, m)
        tau, c = d["tau_true"], d["c_true"]
        Y = c[:, 0:1] * np.exp(-x[None, :] / tau[:, 0:1]) + c[:, 1:2] * np.exp(-x[None, :] / tau[:, 1:2]) + c[:, 2:3]
        Y = Y + 1e-3 * np.abs(Y).max(axis=1, keepdims=True) * np.random.default_rng(7).standard_normal(Y.shape)
    idx = np.arange(B) % Y.shape[0]
    return x, np.ascontiguousarray(Y[idx]), np.ascontiguousarray(g[idx])


def _fit_with(kernel, mdl, Y, x, guess, refit=None):
    bp = vp.BatchProblem(mdl, Y, x=x)
    bp.set_fit_kernel(kernel)
    if refit is not None:
        bp.set_refit(refit)
    a, c, rep = bp.fit(guess)
    out = np.asarray(a).copy(), np.asarray(c).copy(), bp.report_to_numpy(rep).copy()
    bp.close()
    return out


def _assert_same(wave, slots):
    (a0, c0, r0), (a1, c1, r1) = wave, slots
    assert np.array_equal(r0["termination"], r1["termination"])
    assert np.array_equal(r0["n_evals"], r1["n_evals"])
    assert np.array_equal(r0["objective"], r1["objective"], equal_nan=True)
    assert np.array_equal(a0, a1, equal_nan=True)
    assert np.array_equal(np.isnan(c0), np.isnan(c1))
    assert np.nanmax(np.abs(c0 - c1)) <= 1e-13 * np.nanmax(np.abs(c0)), np.nanmax(np.abs(c0 - c1))


def _compare(B, m, grid="uniform"):
    x, Y, g = _batch(B, m, grid)
    mdl = vp.multi_exponential_model(x, g[0])
    wave = _fit_with("wave", mdl, Y, x, g)
    slots = _fit_with("slots", mdl, Y, x, g)
    _assert_same(wave, slots)
    assert slots[2]["n_evals"].min() >= 1  # (every problem was run)


@pytest.mark.parametrize("grid", ["uniform", "log"])
def test_refill_skip_one_wave_groups_queue_runs_dry(grid):
    # four problems per slot of the WHOLE persistent grid and three more: every slot pulls several problems off the queue, the
    # queue runs dry while the waves are mid-fit, and most iterations of a wave finish nothing (the skipped refill section)
    _compare(4 * _grid_slots() + 3, 1024, grid)


@pytest.mark.parametrize("grid", ["uniform", "log"])
def test_refill_skip_three_workgroups_worth_of_slots(grid):
    # 4 x GS x (the waves of three workgroups) + 3 problems: the grid covers them without a refill from the queue -- every pop
    # comes back empty, every wave ends in its lone tail
    _compare(4 * GS * (3 * NG) + 3, 1024, grid)


@pytest.mark.parametrize("B", [1, 2 * GS - 1])
def test_refill_skip_with_empty_slots_and_lone_tail(B):
    _compare(B, 1024)


def test_refill_skip_four_wave_groups_complete():
    # W > 1 (triple exponential at m = 1500 and 2048: four waves per problem, three slots per group -- the only multi-wave slot
    # kernel the library registers), in a process of its own under a time limit: a wave that took the skip branch differently
    # from its partners would hang the workgroup at the next barrier.  That this shape launches fit2_kernel<..., W = 4> is
    # recorded by a kernel trace (profiles/critical_path_w4_kernel_trace.json); the C API has no hook a test could ask
    o = subprocess.run([sys.executable, os.path.join(HERE, "fit2_critical_path_worker.py")], capture_output=True, text=True,
                       timeout=180)
    assert o.returncode == 0 and o.stdout.strip().splitlines()[-1].startswith("OK"), (o.returncode, o.stdout[-500:], o.stderr[-1500:])


@pytest.mark.parametrize("m", [1000, 700])
def test_padded_variants(m):
    # m = 1000: padding in the last register pair (PADM 2); m = 700: general padding (PADM 0)
    _compare(300, m)


def test_flagged_problems_are_still_refitted_by_their_wave():
    # the construction of test_gpu_census.test_refit_of_unrepresentable_jacobians_in_every_kernel_family, slot kernel only: two
    # starts inside the window whose Jacobian the unscaled columns cannot represent, among 64 problems
    m, B = 1024, 64
    d = synth.double_exp_batch(B, m=m, first_problem=4242, noise=1e-3)
    g = d["tau_guess"].copy()
    g[1, 1] = -0.0356
    g[4, 0] = -0.03555
    flagged = (1, 4)
    mdl = vp.multi_exponential_model(d["x"], g[0])
    a0, c0, r0 = _fit_with("slots", mdl, d["Y"], d["x"], g, refit=False)  # what the kernel reports itself
    a1, c1, r1 = _fit_with("slots", mdl, d["Y"], d["x"], g, refit=True)   # ... and with the re-fit at the wave's end
    aw, cw, rw = _fit_with("wave", mdl, d["Y"], d["x"], g, refit=True)
    for b in flagged:
        assert int(r0["termination"][b]) == -2 and int(r0["n_evals"][b]) == 1, (b, r0[b])
        assert np.array_equal(a0[b], g[b])
    rest = np.setdiff1d(np.arange(B), flagged)
    # every problem that is not flagged: bit for bit the same with and without the re-fit, and as the wave kernel
    assert np.array_equal(a1[rest], a0[rest]) and np.array_equal(r1["n_evals"][rest], r0["n_evals"][rest])
    assert np.array_equal(r1["termination"][rest], r0["termination"][rest])
    assert np.array_equal(r1["objective"][rest], r0["objective"][rest], equal_nan=True)
    assert np.array_equal(a1[rest], aw[rest]) and np.array_equal(r1["n_evals"][rest], rw["n_evals"][rest])
    assert np.array_equal(r1["termination"][rest], rw["termination"][rest])
    assert np.array_equal(r1["objective"][rest], rw["objective"][rest], equal_nan=True)
    for b in flagged:  # the re-fit was reached: the oracle's success class and minimum
        p = O.Problem(mdl, d["x"], d["Y"][b])
        p.set_params(g[b])
        ref = p.fit()
        assert (int(r1["termination"][b]) > 0) == (int(ref.termination) > 0), (b, r1[b], ref.termination)
        assert int(r1["n_evals"][b]) > 1
        if int(ref.termination) > 0:
            assert abs(r1["objective"][b] - ref.objective) <= K.REFIT["objective_rel_max"] * ref.objective, (b, r1["objective"][b], ref.objective)
