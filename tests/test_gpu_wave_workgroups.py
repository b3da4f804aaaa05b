"""The slot kernel's one-wave workgroups (vp_fit2.hpp, VP_FIT2_WAVE_WG): the W = 1 slot kernels whose slots fit without the
workgroup's LDS copy of the grid run as workgroups of ONE wave that read the shared grid from global memory (RowSource GMEM).
The grid values, the queue, the static assignment and the arithmetic per problem are unchanged, so every case forces the slot
kernel and compares it BIT FOR BIT with the one-wavefront-per-problem kernel on parameters, termination, evaluation count and
objective, and asks vp_debug_last_fit that the slot kernel was what ran.

Shapes (fp64 double exponential + offset): m = 1024, 1000, 880 -- the full, last-pair and general padding variants of the
16-rows-per-lane set (two slots per wave) -- and m = 512 (8 rows per lane, four slots per wave).  The general variant keeps
its four-group workgroups and their LDS grid (vp_fit2.hpp, fit2_global_grid); its cases hold the same comparison either way.
Batches, with S the slots of the launch (CUs x 8 waves x slots per wave): 3 (statically empty slots, workgroups with nothing
to do), S + 1 (exactly one refill) and 2 S + 17 (refills, a dry queue, lone tails)."""
import numpy as np
import pytest

import fit_cases as FC
import varpro_amd as vp
from stats_cases import case_data, fit_guess
from varpro_amd import synth

pytestmark = pytest.mark.gpu

WAVE, SLOTS = 1, 2  # vp_debug_last_fit: the kernel the launcher issued
SLOTS_PER_WAVE = {1024: 2, 1000: 2, 880: 2, 512: 4}  # fit2_slots at 16 and at 8 fp64 rows per lane
PADDING = {1024: 1, 1000: 2, 880: 0, 512: 1}


def _launch_slots(m):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * SLOTS_PER_WAVE[m]


def _batch(B, m, jitter=False, distinct=512):
    """B double-exponential problems, `distinct` generated ones repeated (a problem's result does not depend on its neighbours);
    jitter: every abscissa moved by up to a fifth of the spacing -- a shared grid that is not uniform, so no recurrence stands in
    for the rows' own grid values"""
    d = synth.double_exp_batch(min(B, distinct), m=m, noise=1e-3)
    x, Y, g = d["x"], d["Y"], d["tau_guess"]
    if jitter:
        rng = np.random.default_rng(11)
        x = x + 0.2 * (x[1] - x[0]) * rng.uniform(-1.0, 1.0, m)
        tau, c = d["tau_true"], d["c_true"]
        Y = c[:, 0:1] * np.exp(-x[None, :] / tau[:, 0:1]) + c[:, 1:2] * np.exp(-x[None, :] / tau[:, 1:2]) + c[:, 2:3]
        Y = Y + 1e-3 * np.abs(Y).max(axis=1, keepdims=True) * rng.standard_normal(Y.shape)
        assert not FC.grid_is_uniform(x)
    idx = np.arange(B) % Y.shape[0]
    return np.ascontiguousarray(x), np.ascontiguousarray(Y[idx]), np.ascontiguousarray(g[idx])


def _fit_with(kernel, mdl, Y, x, guess, padding, refit=None):
    bp = vp.BatchProblem(mdl, Y, x=x)
    bp.set_fit_kernel(kernel)
    if refit is not None:
        bp.set_refit(refit)
    a, _c, rep = bp.fit(guess)
    assert bp.last_fit_kernel() == ((WAVE if kernel == "wave" else SLOTS), padding, 0, 0), bp.last_fit_kernel()
    out = np.asarray(a).copy(), bp.report_to_numpy(rep).copy()
    bp.close()
    return out


def _assert_same(ref, got):
    (a0, r0), (a1, r1) = ref, got
    assert np.array_equal(r0["termination"], r1["termination"])
    assert np.array_equal(r0["n_evals"], r1["n_evals"])
    assert np.array_equal(r0["objective"], r1["objective"], equal_nan=True)
    assert np.array_equal(a0, a1, equal_nan=True)
    assert r1["n_evals"].min() >= 1  # (every problem was run)


def _compare(B, m, jitter=False):
    x, Y, g = _batch(B, m, jitter)
    mdl = vp.multi_exponential_model(x, g[0])
    wave = _fit_with("wave", mdl, Y, x, g, PADDING[m])
    slots = _fit_with("slots", mdl, Y, x, g, PADDING[m])
    _assert_same(wave, slots)
    return x, Y, g, mdl, slots


@pytest.mark.parametrize("batch", ["three", "one_refill", "dry_queue"])
@pytest.mark.parametrize("m", [1024, 1000, 880, 512])
def test_one_wave_workgroups_equal_wave_kernel(m, batch):
    S = _launch_slots(m)
    _compare({"three": 3, "one_refill": S + 1, "dry_queue": 2 * S + 17}[batch], m)


def test_jittered_shared_grid_is_read_row_by_row():
    _compare(_launch_slots(1000) + 1, 1000, jitter=True)


def test_permuted_batch_gives_permuted_results():
    B = 2 * _launch_slots(1024) + 17
    x, Y, g, mdl, (a1, r1) = _compare(B, 1024)
    perm = np.random.default_rng(3).permutation(B)
    a2, r2 = _fit_with("slots", mdl, Y[perm], x, g[perm], 1)
    _assert_same((a1[perm], r1[perm]), (a2, r2))


def test_two_handles_on_two_streams_interleaved():
    import torch
    dev = torch.device("cuda", 0)
    B, m = _launch_slots(1024) + 1, 1024
    streams = [torch.cuda.current_stream(dev), torch.cuda.Stream(device=dev)]
    data, alone, hs, gs = [], [], [], []
    for i in range(2):
        d = synth.double_exp_batch(512, m=m, first_problem=1000 * i, noise=1e-3)
        idx = np.arange(B) % 512
        x, Y, g = d["x"], np.ascontiguousarray(d["Y"][idx]), np.ascontiguousarray(d["tau_guess"][idx])
        mdl = vp.multi_exponential_model(x, g[0])
        data.append((mdl, x, Y, g))
        alone.append(_fit_with("slots", mdl, Y, x, g, 1))
    for i, (mdl, x, Y, g) in enumerate(data):
        with torch.cuda.stream(streams[i]):
            bp = vp.BatchProblem(mdl, torch.from_numpy(Y).to(dev), x=torch.from_numpy(x).to(dev))
            bp.set_fit_kernel("slots")
            hs.append(bp)
            gs.append(torch.from_numpy(g).to(dev))
    torch.cuda.synchronize()
    outs = [None, None]
    for k in range(4):  # no synchronisation between the launches: the second handle's workgroups move in as the first's drain
        i = k % 2
        with torch.cuda.stream(streams[i]):
            outs[i] = hs[i].fit(gs[i], want_coefficients=False)
    torch.cuda.synchronize()
    for i in range(2):
        assert hs[i].last_fit_kernel() == (SLOTS, 1, 0, 0)
        a, _c, rep = outs[i]
        _assert_same(alone[i], (a.cpu().numpy(), hs[i].report_to_numpy(rep)))
        hs[i].close()


def test_flagged_problem_is_refitted_with_the_global_grid():
    # the construction of test_gpu_fit2_critical_path.test_flagged_problems_are_still_refitted_by_their_wave: two starts inside
    # the window whose Jacobian the unscaled columns cannot represent; the wave that flagged them re-fits them at its end
    # (fit2_refit_flagged), reading the grid from where the slot loop read it
    m, B = 1024, 64
    d = synth.double_exp_batch(B, m=m, first_problem=4242, noise=1e-3)
    g = d["tau_guess"].copy()
    g[1, 1] = -0.0356
    g[4, 0] = -0.03555
    mdl = vp.multi_exponential_model(d["x"], g[0])
    a0, r0 = _fit_with("slots", mdl, d["Y"], d["x"], g, 1, refit=False)
    for b in (1, 4):  # flagged: what the slot loop reports itself
        assert int(r0["termination"][b]) == -2 and int(r0["n_evals"][b]) == 1, (b, r0[b])
    wave = _fit_with("wave", mdl, d["Y"], d["x"], g, 1, refit=True)
    slots = _fit_with("slots", mdl, d["Y"], d["x"], g, 1, refit=True)
    for b in (1, 4):  # ... and the re-fit was reached
        assert int(slots[1]["n_evals"][b]) > 1
    _assert_same(wave, slots)


def test_no_set_changed_its_launcher():
    """vp_debug_last_fit after a fit under "slots" against the table of tests/fit_cases.py, for every case whose set has the
    slot launcher (the record needs a handle, so this runs on the device): slots where the table says slots, with its padding
    variant, and the wave kernel where it says so -- the weighted cases, the per-problem grids and the set without room"""
    cases = [fc for fc in FC.FIT_CASES if fc.slots is not None]
    assert len(cases) > 40 and any(fc.slots[0] == WAVE for fc in cases) and any(fc.slots[0] == SLOTS for fc in cases)
    for fc in cases:
        c = fc.case
        d = case_data(c)
        bp = vp.BatchProblem(d["model"], d["Y"], x=d["x"], weights=d["w"])
        bp.set_fit_kernel("slots")
        bp.fit(fit_guess(c))
        assert bp.last_fit_kernel() == fc.slots, (FC.fit_case_id(fc), bp.last_fit_kernel(), fc.slots)
        bp.close()
