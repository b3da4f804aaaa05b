"""CPU tier of box bounds on the nonlinear parameters (vp_set_bounds, VP_FLAG_DEVICE_COLUMNS): the numpy mirror of the
transform alpha = g(u) (varpro_amd/bounds.py; the device's copy is bound_map / bound_unmap of varpro_amd/csrc/vp_cols.hpp),
the argument checks of BatchProblem.set_bounds, and the constants of the header's mirrors.  The GPU tier is
tests/test_gpu_bounds.py."""
import os
import re

import numpy as np
import pytest

import varpro_amd as vp
from varpro_amd import _lib, bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf
# one parameter of each kind: none, lo and hi, lo only, hi only
LO = np.array([-INF, 0.5, 2.0, -INF])
HI = np.array([INF, 3.0, INF, -1.0])


def test_round_trip_for_all_four_bound_types():
    rng = np.random.default_rng(1)
    a = np.stack([rng.uniform(-5, 5, 200), rng.uniform(0.5, 3.0, 200), 2.0 + rng.uniform(0, 50, 200),
                  -1.0 - rng.uniform(0, 50, 200)], 1)
    u = bounds.to_internal(a, LO, HI)
    back = bounds.from_internal(u, LO, HI)
    # (asin amplifies the rounding of its argument by 1 / cos u near a bound, g damps it by cos u again: a few eps |alpha|)
    assert np.abs(back - a).max() <= 16 * np.finfo(np.float64).eps * 52  # |alpha| <= 52
    assert np.array_equal(back[:, 0], a[:, 0]) and np.array_equal(u[:, 0], a[:, 0])
    # points ON a bound come back exactly, points outside are clamped onto it first
    edge = np.array([[7.0, 0.5, 2.0, -1.0], [7.0, 3.0, 2.0, -1.0], [-7.0, 0.0, 1.0, 0.0], [0.0, 9.0, -3.0, 5.0]])
    want = np.array([[7.0, 0.5, 2.0, -1.0], [7.0, 3.0, 2.0, -1.0], [-7.0, 0.5, 2.0, -1.0], [0.0, 3.0, 2.0, -1.0]])
    assert np.array_equal(bounds.from_internal(bounds.to_internal(edge, LO, HI), LO, HI), want)
    # per-problem boxes broadcast like shared ones
    lo2, hi2 = np.tile(LO, (200, 1)), np.tile(HI, (200, 1))
    assert np.array_equal(bounds.to_internal(a, lo2, hi2), u)
    assert np.isnan(bounds.from_internal(np.full(4, np.nan), LO, HI)).all()  # a NaN stays a NaN, it is not clamped away


def test_results_lie_within_the_box_bounds_included():
    rng = np.random.default_rng(2)
    u = np.concatenate([rng.uniform(-1e8, 1e8, (4000, 4)), rng.uniform(-10, 10, (4000, 4)),
                        np.array([[0.0] * 4, [1e8] * 4, [-1e8] * 4, [np.pi / 2] * 4, [-np.pi / 2] * 4, [1e-300] * 4])])
    for lo, hi in ((LO, HI), (np.array([-INF, 1e-3, 1e6, -INF]), np.array([INF, 1e-3 * (1 + 1e-12), INF, -1e6]))):
        a = bounds.from_internal(u, lo, hi)
        assert (a >= lo).all() and (a <= hi).all()
        assert np.isfinite(bounds.dalpha_du(u, lo, hi)).all()


def test_a_guess_far_from_a_one_sided_bound_maps_without_overflow():
    """(alpha - lo + 1)^2 overflows beyond 1.3e154: the map is formed without the square, in both directions"""
    lo, hi = np.array([2.0, -INF]), np.array([INF, -1.0])
    a = np.array([[1e200, -1e200], [1e300, -1e300], [3e154, -3e154]])
    u = bounds.to_internal(a, lo, hi)
    assert np.isfinite(u).all()
    back = bounds.from_internal(u, lo, hi)
    assert (np.abs(back / a - 1) <= 4 * np.finfo(np.float64).eps).all()  # two roots, a product, an addition: a few eps
    assert np.array_equal(np.abs(bounds.dalpha_du(u, lo, hi)), np.ones((3, 2)))


def test_derivative_agrees_with_a_central_difference():
    rng = np.random.default_rng(3)
    u = rng.uniform(-6, 6, (500, 4))
    h = 1e-6
    fd = (bounds.from_internal(u + h, LO, HI) - bounds.from_internal(u - h, LO, HI)) / (2 * h)
    d = bounds.dalpha_du(u, LO, HI)
    # central difference: h^2 |g'''| / 6 + eps |g| / h, with |g'''| <= (hi - lo)/2 = 1.25 resp. <= 1 and |g| <= 9
    assert np.abs(fd - d).max() <= 1e-12 * 1.25 + 2.3e-16 * 9 / h * 4
    assert np.array_equal(d[:, 0], np.ones(500))


class _Handle(vp.BatchProblem):
    """a BatchProblem without a device handle: set_bounds must refuse bad arguments before it touches the library"""

    def __init__(self, B, q):
        self.B, self.q = B, q
        self._h = None

        class _NoLib:
            def __getattr__(self, name):
                raise AssertionError("the library was touched: %s" % name)
        self.lib = _NoLib()
        self.device_mode = False


def test_set_bounds_refuses_bad_arguments_without_a_gpu():
    bp = _Handle(B=3, q=2)
    bad = [(np.zeros(3), np.ones(3)),                    # wrong length
           (np.zeros((2, 2)), np.ones((2, 2))),          # wrong batch size
           (np.zeros((3, 2, 1)), None),                  # wrong rank
           ([0.0, np.nan], [1.0, 2.0]),                  # NaN
           (None, [1.0, np.nan]),
           ([0.0, 1.0], [1.0, 1.0]),                     # lo == hi: fixing a parameter is not supported
           ([0.0, 2.0], [1.0, 1.0]),                     # lo > hi
           (np.zeros((3, 2)), np.array([1.0, 0.0])),     # (B, q) against (q,): one column empty
           ([INF, 0.0], None), (None, [-INF, 0.0])]      # an empty half line
    for lower, upper in bad:
        with pytest.raises(ValueError):
            bp.set_bounds(lower, upper)
    # what reaches the library: float64, contiguous, (q,) or (B, q); None on a side is infinite
    lo, hi, per = bounds.normalize([0.0, 1.0], None, 3, 2)
    assert not per and lo.dtype == np.float64 and np.array_equal(lo, [0.0, 1.0]) and np.array_equal(hi, [INF, INF])
    lo, hi, per = bounds.normalize(np.array([0, 1], dtype=np.int32), np.full((3, 2), 5.0, dtype=np.float32), 3, 2)
    assert per and lo.shape == hi.shape == (3, 2) and lo.flags["C_CONTIGUOUS"] and lo.dtype == hi.dtype == np.float64
    assert bounds.normalize(None, None, 3, 2) is None


def test_flag_and_symbol_match_the_header():
    header = open(os.path.join(ROOT, "include", "varpro_hip.h")).read()
    flags = dict((k, int(v)) for k, v in re.findall(r"\bVP_FLAG_([A-Z_]+) = 1 << (\d+)", header))
    assert flags["DEVICE_COLUMNS"] == 6 and _lib.VP_FLAG_DEVICE_COLUMNS == 1 << 6
    assert len(set(flags.values())) == len(flags)
    for name, bit in flags.items():
        assert getattr(_lib, "VP_FLAG_" + name) == 1 << bit
    assert re.search(r"int vp_set_bounds\(vp_batch \*h, const double \*lower, const double \*upper, int per_problem\);", header)
    assert "vp_set_bounds" in _lib.ABI_SYMBOLS
    lib = vp.load_library()
    assert hasattr(lib, "vp_set_bounds") and len(lib.vp_set_bounds.argtypes) == 4
    rust = open(os.path.join(ROOT, "bindings", "rust", "varpro_hip.rs")).read()
    assert re.search(r"VP_FLAG_DEVICE_COLUMNS: i32 = 64;", rust)
    assert re.search(r"pub fn vp_set_bounds\(h: \*mut vp_batch, lower: \*const f64, upper: \*const f64, per_problem: i32\) -> i32;", rust)
    cpp = open(os.path.join(ROOT, "varpro_amd", "cpp", "varpro.hpp")).read()
    assert "vp_set_bounds" in cpp and "VP_FLAG_DEVICE_COLUMNS" in cpp
    # a null handle is refused by the library itself, without a device
    assert lib.vp_set_bounds(None, None, None, 0) == _lib.VP_ERR_INVALID
