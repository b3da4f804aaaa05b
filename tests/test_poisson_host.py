"""CPU tier of the Poisson-weighted fits (vp_set_weights, vp_poisson_reweight, BatchProblem.fit_poisson): the symbols, what
the Python layer refuses without a device, and the reference of the GPU tier checking itself -- the CPU iterated fit of
tests/poisson_cases.py ends at the Poisson score equations, the Neyman fit it starts from does not."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import poisson_cases as pc
import varpro_amd as vp
from varpro_amd import _lib
from varpro_amd.batch import POISSON_ROUNDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The bound on the normalised score of the CPU iterated fit after POISSON_ROUNDS rounds, from that run's own convergence
# sequence: the largest score over both workloads falls by a factor of 5 to 8 per round -- 2.8e-1,
# 4.0e-2, 5.8e-3, 9.3e-4, 1.4e-4, 2.2e-5, 3.4e-6, 4.9e-7 -- and stops at 1.8e-7 (double exponential) and 1.4e-7 (lifetime)
# from round 9 on (round 10 repeats round 9: what fits that end on ftol = 30 eps leave).  The bound is one contraction
# step above that floor.
SCORE_BOUND = 1e-6
# ... and the largest relative parameter change between rounds at which the sequence counts as converged: the accuracy of
# the parameters of a fit that ends on ftol = 30 eps, sqrt(ftol) = 8e-8 -- the 1e-7 the project's smoke run holds its
# parameters to for the same reason
ALPHA_NOISE = 1e-7


def test_symbols_are_listed_exported_and_mirrored():
    lib = vp.load_library()
    for name in ("vp_set_weights", "vp_poisson_reweight"):
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name)
    assert (_lib.VP_POISSON_NEYMAN, _lib.VP_POISSON_MODEL) == (0, 1)
    header = open(os.path.join(ROOT, "include", "varpro_hip.h")).read()
    assert "VP_POISSON_NEYMAN = 0, VP_POISSON_MODEL = 1" in header
    rust = open(os.path.join(ROOT, "bindings", "rust", "varpro_hip.rs")).read()
    assert "pub fn vp_set_weights(" in rust and "pub fn vp_poisson_reweight(" in rust
    cpp = open(os.path.join(ROOT, "varpro_amd", "cpp", "varpro.hpp")).read()
    for name in ("vp_set_weights(", "vp_poisson_reweight(", "fit_poisson(", "neyman_weights("):
        assert name in cpp, name


def test_a_null_handle_is_refused():
    lib = vp.load_library()
    y = np.ones(4)
    p = C.c_void_p(y.ctypes.data)
    assert lib.vp_set_weights(None, p, p) == _lib.VP_ERR_INVALID
    assert lib.vp_poisson_reweight(None, p, _lib.VP_POISSON_NEYMAN, C.c_double(1.0), None, None) == _lib.VP_ERR_INVALID


class _NoDevice(vp.BatchProblem):
    """the Python layer of a handle without the handle: the argument checks run before the ABI is reached"""

    def __init__(self, B, m, S=1, weighted=True, w_per_problem=True):
        self.lib, self._h, self.device_mode = None, None, False
        self.B, self.S, self.m, self.n, self.q = B, S, m, 3, 2
        self.single_rhs = S == 1
        self.np_dtype = np.dtype(np.float64)
        self.weighted, self.w_per_problem = weighted, w_per_problem
        self._have_params = False


def test_python_argument_validation():
    B, m = 3, 8
    Y = np.ones((B, m))
    bp = _NoDevice(B, m)
    for bad in (dict(mode="pearson"), dict(floor=0.0), dict(floor=-1.0), dict(floor=np.inf), dict(floor=np.nan)):
        with pytest.raises(ValueError):
            bp.poisson_reweight(Y, **{"mode": "neyman", **bad})
    with pytest.raises(ValueError):
        bp.poisson_reweight(np.ones((B, m + 1)), "neyman")
    with pytest.raises(ValueError):  # model mode before any parameters
        bp.poisson_reweight(Y, "model")
    with pytest.raises(ValueError):  # weights per right-hand side do not exist
        _NoDevice(B, m, S=2).poisson_reweight(np.ones((B, 2, m)), "neyman")
    with pytest.raises(ValueError):  # shared weights
        _NoDevice(B, m, w_per_problem=False).poisson_reweight(Y, "neyman")
    with pytest.raises(ValueError):  # a handle without weights
        _NoDevice(B, m, weighted=False, w_per_problem=False).set_weights(np.ones(m), Y)
    with pytest.raises(ValueError):  # the layout of creation stays
        bp.set_weights(np.ones(m), Y)
    with pytest.raises(ValueError):
        _NoDevice(B, m, w_per_problem=False).set_weights(np.ones((B, m)), Y)
    with pytest.raises(ValueError):
        bp.set_weights(np.ones((B, m)), np.ones((B, m + 1)))
    with pytest.raises(ValueError):
        bp.fit_poisson(Y, np.ones((B, 2)), rounds=-1)


def test_the_mirror_against_plain_formulas():
    rng = np.random.default_rng(5)
    Y = rng.poisson(3.0, (4, 33)).astype(np.float64)
    F = rng.uniform(-0.5, 6.0, (4, 33))
    w, yw = pc.reweight_mirror(Y, None)
    assert np.array_equal(w, 1 / np.sqrt(np.maximum(Y, 1.0))) and np.array_equal(yw, w * Y) and (Y == 0).any()
    w, yw = pc.reweight_mirror(Y, F)
    ft = np.maximum(F, 1.0)
    assert np.array_equal(w, 1 / np.sqrt(ft)) and (F < 0).any()
    D, X, TD, TX = pc.goodness_mirror(Y, F)
    Dn = 2 * (np.where(Y > 0, Y * np.log(np.where(Y > 0, Y, 1) / ft), 0) - (Y - ft)).sum(1)
    assert np.allclose(np.asarray(D, dtype=np.float64), Dn, rtol=1e-13) and (np.asarray(D) >= 0).all()
    assert np.allclose(np.asarray(X, dtype=np.float64), ((Y - ft) ** 2 / ft).sum(1), rtol=1e-13)
    # non-finite input goes through to w and Y_w
    Y[1, 3], F[2, 4], F[3, 5] = np.nan, np.nan, np.inf
    w, yw = pc.reweight_mirror(Y, None)
    assert np.isnan(w[1, 3]) and np.isnan(yw[1, 3]) and np.isfinite(w[0]).all()
    w, yw = pc.reweight_mirror(Y, F)
    assert np.isnan(w[2, 4]) and np.isnan(w[3, 5]) and np.isnan(yw[3, 5])
    # fp32: every operation in fp32
    w32, yw32 = pc.reweight_mirror(Y[0], F[0], dtype=np.float32)
    assert w32.dtype == np.float32 and yw32.dtype == np.float32


@functools.lru_cache(maxsize=None)
def _sequence(name):
    wl = pc.double_exp(pc.DOUBLE_EXP_SEED, pc.B_FIT) if name == "double_exp" else pc.lifetime(pc.LIFETIME_SEED, pc.B_FIT)
    return wl, pc.iterated_fit(wl, POISSON_ROUNDS + 1)


@pytest.mark.parametrize("name", ["double_exp", "lifetime"])
def test_the_cpu_iterated_fit_ends_at_the_poisson_score_equations(name):
    wl, seq = _sequence(name)
    # the workloads are what the issue asks for: low counts, empty bins, fits under the floor
    assert wl.Y.max(1).min() < 50 and wl.Y.max(1).max() > 200
    assert (wl.Y == 0).mean() > 0.1 and (pc.best_fit(wl, seq[-1][0], seq[-1][1]) < pc.FLOOR).mean() > 0.1
    # every fit of every round succeeds on the oracle: no problem is excluded anywhere
    for a, C, term in seq:
        assert (term > 0).all() and np.isfinite(a).all() and np.isfinite(C).all()
    change = [pc.relative_change(seq[r][0], seq[r - 1][0]).max() for r in range(1, len(seq))]
    score = [pc.normalised_score(wl, a, C).max() for a, C, _t in seq]
    print("%s: max relative change of alpha per round %s" % (name, " ".join("%.2e" % c for c in change)))
    print("%s: max normalised score after each fit   %s" % (name, " ".join("%.2e" % s for s in score)))
    # the default number of rounds is the first at which the parameters stop moving beyond the LM's own stopping noise
    assert change[POISSON_ROUNDS - 1] <= ALPHA_NOISE and change[POISSON_ROUNDS] <= ALPHA_NOISE
    assert score[POISSON_ROUNDS] <= SCORE_BOUND
    # ... and the bound discriminates: the Neyman fit the iteration starts from misses it by six orders of magnitude
    neyman = pc.normalised_score(wl, seq[0][0], seq[0][1])
    assert neyman.min() >= 1e5 * SCORE_BOUND and np.median(neyman) >= 1e6 * SCORE_BOUND, (neyman.min(), np.median(neyman))


def test_the_default_is_the_smallest_such_count():
    """over both workloads together: one round fewer leaves a parameter change above the stopping noise"""
    worst = []
    for name in ("double_exp", "lifetime"):
        _wl, seq = _sequence(name)
        worst.append([pc.relative_change(seq[r][0], seq[r - 1][0]).max() for r in range(1, len(seq))])
    worst = np.max(np.array(worst), 0)
    assert worst[POISSON_ROUNDS - 1] <= ALPHA_NOISE < worst[POISSON_ROUNDS - 2], worst
