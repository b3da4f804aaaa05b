"""CPU tier of the robust fits (vp_robust_reweight, vp_weights, BatchProblem.fit_robust): the symbols, what is refused
without a device, the numpy mirror against plain formulas, and the reference of the GPU tier checking itself -- the CPU
iterated fit of tests/robust_cases.py ends at the M-estimating equations and resists the outliers the plain fit does not."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import robust_cases as rc
import varpro_amd as vp
from varpro_amd import _lib
from varpro_amd.batch import ROBUST_ROUNDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The bound on the normalised score after ROBUST_ROUNDS rounds: a ten-thousandth of a standard deviation of each component
# of the estimating equations -- a design choice far below the statistical error of the estimate, not a measurement.
ROBUST_SCORE_BOUND = 1e-4
# The CPU sequences contract linearly: the largest score of a batch falls per round by 0.38 (double
# exponential, Huber), 0.45 (lifetime, both losses) and 0.59 (double exponential, Tukey) once the first rounds are over.
# The GPU tier uses the largest, rounded up.
CONTRACTION = 0.6
LOSSES = ("huber", "tukey")
NAMES = ("double_exp", "lifetime")


def test_symbols_are_listed_exported_and_mirrored():
    lib = vp.load_library()
    for name in ("vp_robust_reweight", "vp_weights"):
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name)
    assert (_lib.VP_ROBUST_HUBER, _lib.VP_ROBUST_CAUCHY, _lib.VP_ROBUST_TUKEY) == (0, 1, 2)
    header = open(os.path.join(ROOT, "include", "varpro_hip.h")).read()
    assert "VP_ROBUST_HUBER = 0, VP_ROBUST_CAUCHY = 1, VP_ROBUST_TUKEY = 2" in header
    assert "int vp_robust_reweight(" in header and "int vp_weights(" in header
    rust = open(os.path.join(ROOT, "bindings", "rust", "varpro_hip.rs")).read()
    assert "pub fn vp_robust_reweight(" in rust and "pub fn vp_weights(" in rust
    for line in ("VP_ROBUST_HUBER: i32 = 0", "VP_ROBUST_CAUCHY: i32 = 1", "VP_ROBUST_TUKEY: i32 = 2"):
        assert line in rust
    cpp = open(os.path.join(ROOT, "varpro_amd", "cpp", "varpro.hpp")).read()
    for name in ("vp_robust_reweight(", "vp_weights(", "robust_reweight(", "fit_robust(", "weights()"):
        assert name in cpp, name
    assert "kRobustRounds = %d;" % ROBUST_ROUNDS in cpp


def test_a_null_handle_is_refused():
    lib = vp.load_library()
    y = np.ones(4)
    p = C.c_void_p(y.ctypes.data)
    assert lib.vp_robust_reweight(None, p, p, _lib.VP_ROBUST_HUBER, C.c_double(0.0), C.c_double(0.0), None, None) == _lib.VP_ERR_INVALID
    assert lib.vp_weights(None, p) == _lib.VP_ERR_INVALID


class _NoDevice(vp.BatchProblem):
    """the Python layer of a handle without the handle: the argument checks run before the ABI is reached"""

    def __init__(self, B, m, S=1, weighted=True, w_per_problem=True):
        self.lib, self._h, self.device_mode = None, None, False
        self.B, self.S, self.m, self.n, self.q = B, S, m, 3, 2
        self.single_rhs = S == 1
        self.np_dtype = np.dtype(np.float64)
        self.weighted, self.w_per_problem = weighted, w_per_problem
        self._have_params = True


def test_python_argument_validation():
    B, m = 3, 8
    Y = np.ones((B, m))
    bp = _NoDevice(B, m)
    bad_arguments = [dict(loss="l1"), dict(loss=0)]
    bad_arguments += [dict(tuning=v) for v in (-1.0, np.inf, np.nan)] + [dict(scale=v) for v in (-1.0, np.inf, np.nan)]
    for bad in bad_arguments:
        with pytest.raises(ValueError):
            bp.robust_reweight(Y, **bad)
        with pytest.raises(ValueError):
            bp.fit_robust(Y, np.ones((B, 2)), **bad)
    with pytest.raises(ValueError):
        bp.robust_reweight(np.ones((B, m + 1)))
    with pytest.raises(ValueError):
        bp.robust_reweight(Y, base_weights=np.ones(m))
    with pytest.raises(ValueError):  # weights per right-hand side do not exist
        _NoDevice(B, m, S=2).robust_reweight(np.ones((B, 2, m)))
    with pytest.raises(ValueError):  # shared weights
        _NoDevice(B, m, w_per_problem=False).robust_reweight(Y)
    with pytest.raises(ValueError):  # a handle without weights
        _NoDevice(B, m, weighted=False, w_per_problem=False).robust_reweight(Y)
    with pytest.raises(ValueError):
        _NoDevice(B, m, weighted=False, w_per_problem=False).weights()
    with pytest.raises(ValueError):
        bp.fit_robust(Y, np.ones((B, 2)), rounds=-1)
    nofit = _NoDevice(B, m)
    nofit._have_params = False
    with pytest.raises(ValueError):  # before any parameters
        nofit.robust_reweight(Y)


@pytest.mark.parametrize("loss", ["huber", "cauchy", "tukey"])
def test_the_mirror_against_plain_formulas(loss):
    k = rc.K95[loss]
    u = np.linspace(1e-3, 3 * k, 4001)
    omega = rc.sqrt_omega(u, loss, k, np.float64) ** 2
    # psi = u omega is the derivative of rho
    h = 1e-6
    rho = lambda v: np.asarray(rc.rho_mirror(v[:, None], loss, k)[0], np.float64)  # noqa: E731
    drho = (rho(u + h) - rho(u - h)) / (2 * h)
    assert np.abs(drho - u * omega).max() <= 1e-8 * k
    # omega is continuous at |u| = k, 1 at 0, never above 1 and falls with |u|
    below, above = rc.sqrt_omega(np.array([k * (1 - 1e-12), k * (1 + 1e-12)]), loss, k, np.float64) ** 2
    assert abs(below - above) <= 1e-11
    assert rc.sqrt_omega(np.zeros(1), loss, k, np.float64)[0] == 1.0
    assert (omega <= 1.0).all() and (np.diff(omega) <= 0).all()
    if loss == "tukey":
        assert (omega[u >= k] == 0).all()


def test_the_mirror_of_the_scale():
    rng = np.random.default_rng(8)
    for m in (1, 2, 7, 64, 201):
        e = rng.standard_normal((5, m))
        w0 = np.ones((5, m))
        s = rc.scale_mirror(e, w0, np.float64)
        assert np.allclose(s, rc.MAD_TO_SIGMA * np.median(np.abs(e), 1), rtol=1e-15)
    # rows of weight 0 do not count: me even in one problem, odd in the other
    e = np.array([[3.0, 0.0, 1.0, 0.0, 2.0, 4.0], [3.0, 0.0, 1.0, 0.0, 2.0, 0.0]])
    w0 = (e != 0).astype(np.float64)
    assert np.array_equal(rc.scale_mirror(e, w0, np.float64), rc.MAD_TO_SIGMA * np.array([2.5, 2.0]))
    assert np.array_equal(rc.scale_mirror(e, np.zeros_like(e), np.float64), [0.0, 0.0])
    e[1, 2] = np.inf
    assert np.isnan(rc.scale_mirror(e, w0, np.float64)[1])
    # the whole mirror: s == 0 keeps the base weights, a NaN goes through, fp32 stays fp32
    Y, F = rng.standard_normal((3, 9)), np.zeros((3, 9))
    Y[1, :6] = 0.0
    Y[2, 4] = np.nan
    base = rng.uniform(0.5, 1.5, (3, 9))
    for loss in ("huber", "cauchy", "tukey"):
        w, yw, s, u = rc.reweight_mirror(Y, F, base, loss, rc.K95[loss], 0.0)
        assert s[1] == 0 and np.array_equal(w[1], base[1]) and np.array_equal(yw[1], base[1] * Y[1])
        assert np.isnan(s[2]) and np.isnan(w[2]).all() and np.isfinite(w[0]).all() and (w[0] <= base[0]).all()
        w32 = rc.reweight_mirror(Y, F, base, loss, rc.K95[loss], 0.0, np.float32)
        assert all(a.dtype == np.float32 for a in w32)
        wf, _ywf, sf, _uf = rc.reweight_mirror(Y, F, base, loss, rc.K95[loss], 0.75)
        assert (sf == 0.75).all() and np.isnan(wf[2, 4]) and np.isfinite(np.delete(wf[2], 4)).all()


@functools.lru_cache(maxsize=None)
def _sequence(name, loss):
    wl = rc.workload(name)
    return wl, rc.iterated_fit(wl, loss, ROBUST_ROUNDS)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", NAMES)
def test_the_cpu_iterated_fit_ends_at_the_estimating_equations(name, loss):
    wl, seq = _sequence(name, loss)
    assert 0.04 < wl.spiked.mean() < 0.06 and (wl.Y >= wl.clean).all() and np.array_equal(wl.Y, np.rint(wl.Y))
    # every fit of every round succeeds on the oracle: no problem is excluded anywhere
    for a, Cc, term in seq:
        assert (term > 0).all() and np.isfinite(a).all() and np.isfinite(Cc).all()
    score = [rc.normalised_score(wl, a, Cc, loss).max() for a, Cc, _t in seq]
    print("%s/%s: max normalised score after each fit %s" % (name, loss, " ".join("%.2e" % s for s in score)))
    assert score[ROBUST_ROUNDS] <= ROBUST_SCORE_BOUND
    # the contraction factor the GPU tier's allowance uses covers the last rounds of every sequence
    assert max(score[r + 1] / score[r] for r in range(ROBUST_ROUNDS - 4, ROBUST_ROUNDS)) <= CONTRACTION
    # ... and the bound discriminates: the fit at the base weights misses it by four orders of magnitude
    assert rc.normalised_score(wl, seq[0][0], seq[0][1], loss).min() >= 1e3 * ROBUST_SCORE_BOUND


def test_the_default_is_the_smallest_such_count():
    """over all four sequences together: one round fewer leaves a problem outside the bound"""
    worst = np.max([[rc.normalised_score(wl, a, Cc, loss).max() for a, Cc, _t in seq]
                    for wl, seq, loss in (_sequence(name, loss) + (loss,) for name in NAMES for loss in LOSSES)], 0)
    assert worst[ROBUST_ROUNDS] <= ROBUST_SCORE_BOUND < worst[ROBUST_ROUNDS - 1], worst


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", NAMES)
def test_outlier_resistance(name, loss):
    wl, seq = _sequence(name, loss)
    plain, robust = rc.parameter_error(wl, seq[0][0]), rc.parameter_error(wl, seq[ROBUST_ROUNDS][0])
    print("%s/%s: median relative parameter error %.4f at the base weights, %.4f after %d rounds" % (name, loss, plain, robust, ROBUST_ROUNDS))
    assert robust < plain
    # the weights are the outlier map: the spiked bins are the ones that lose their weight
    W = rc.reweight_mirror(wl.Y, rc.pc.best_fit(wl, seq[-1][0], seq[-1][1]), wl.w0, loss, rc.K95[loss], 0.0)[0]
    kept = W / wl.w0
    assert np.median(kept[wl.spiked]) < 0.75 and np.median(kept[~wl.spiked]) > 0.9  # (omega < 0.56 against omega > 0.81)
