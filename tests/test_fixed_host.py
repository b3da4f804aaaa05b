"""CPU tier of fixed nonlinear parameters (vp_batch_create_fixed, vp_set_fixed_values; BatchProblem(fixed=...)): the numpy
mirror of the reduced model against the full one, the oracle on the reduced closures (the condition the GPU tier's contract
presupposes: it succeeds on every problem of every fit case), the declarations of the two entry points in every binding,
and the Python-side bookkeeping between the full parameter order and the handle's reduced one, on arrays without a device.
The GPU tier is tests/test_gpu_fixed.py."""
import os
import re

import numpy as np
import pytest

import fixed_cases as fc
import varpro_amd as vp
from varpro_amd import _lib, fixed
from test_gpu_extfit import oracle_fits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("key", fc.CASE_KEYS)
def test_reduced_mirror_equals_the_full_mirror_at_the_expanded_point(key):
    case, _x, alpha = fc.columns_case(key, 37, B=4)
    red = case.reduced(alpha[0])
    a_free = alpha[:, case.free]
    full_at = red.expand(a_free)
    assert np.array_equal(full_at[:, case.free], a_free) and np.array_equal(full_at[:, case.held], np.tile(alpha[0, case.held], (4, 1)))
    assert np.array_equal(red.eval_batch(a_free), case.cm.eval_batch(full_at))
    assert np.array_equal(red.derivs_batch(a_free), case.cm.derivs_batch(full_at)[:, case.free_pairs])
    # the reduced pair table: the free pairs in model order, parameters renumbered over the free ones
    want = [(j, case.free.index(k)) for j, k in case.cm.pairs() if k in case.free]
    assert red.pairs() == want and red.shape().n_params == len(case.free) and len(want) == len(case.free_pairs)


def test_the_trap_case_is_the_trap_the_issue_describes():
    case, _x, _alpha = fc.columns_case("d", 16)
    mdl = case.model()
    held = set(case.held)
    per_function = [[pi for j, _a, pi in mdl.pairs if j == f] for f in range(mdl.base_function_count())]
    all_fixed = [f for f, ps in enumerate(per_function) if ps and all(p in held for p in ps)]
    has_free = [f for f, ps in enumerate(per_function) if any(p not in held for p in ps)]
    assert any(min(has_free) < f < max(has_free) for f in all_fixed)       # all fixed, between two functions with free ones
    irf_f = [f for f, k in enumerate(mdl.kinds) if k == vp.basis.EXP_DECAY_IRF]
    assert irf_f and all(f in has_free and f > max(all_fixed) for f in irf_f)  # a free tau behind it
    assert any(f > irf_f[0] and mdl.kinds[f] not in vp.basis.IRF_KINDS for f in has_free)  # a pointwise run behind the IRF function
    shared = [p for p in held if sum(p in ps for ps in per_function) == 2]
    assert shared                                                              # one parameter of two functions, fixed


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("key", fc.FIT_KEYS)
def test_the_oracle_succeeds_on_every_problem_of_every_fit_case(key, weighted):
    ref = fc.fit_reference(key, weighted)
    assert ref[1].shape == (fc.B_FIT,) and (ref[1] > 0).all(), np.nonzero(ref[1] <= 0)[0]


@pytest.mark.parametrize("key", fc.FIT_KEYS)
def test_fixing_at_the_free_optimum_reproduces_its_objective(key):
    case, _x, Y, guess, _values, _w = fc.fit_case(key)
    sel = slice(0, 8)
    a_full, term, _nev, obj = oracle_fits(case.cm, Y[sel], guess[sel])
    assert (term > 0).all()
    values = np.zeros_like(a_full)
    values[:, case.held] = a_full[:, case.held]
    a_red, term_r, _nev_r, obj_r = fc.reduced_oracle_fits(case, Y[sel], guess[sel], values)
    assert (term_r > 0).all()
    rel = np.abs(obj_r - obj) / obj
    assert rel.max() <= 1e-10, rel


def test_both_entry_points_are_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "varpro_hip.h")).read()
    assert re.search(r"int vp_batch_create_fixed\(vp_batch \*\*out, const vp_model_desc \*model, int dtype, int64_t m, int64_t S, "
                     r"int64_t B, const void \*t,\s+const void \*Y, const void \*w, double svd_epsilon, int flags, int device, "
                     r"void \*hip_stream,\s+const int32_t \*fixed, const double \*values, int per_problem\);", header)
    assert re.search(r"int vp_set_fixed_values\(vp_batch \*h, const double \*values, int per_problem\);", header)
    assert "vp_batch_create_fixed" in _lib.ABI_SYMBOLS and "vp_set_fixed_values" in _lib.ABI_SYMBOLS
    lib = vp.load_library()
    assert len(lib.vp_batch_create_fixed.argtypes) == 16 and len(lib.vp_set_fixed_values.argtypes) == 3
    rust = open(os.path.join(ROOT, "bindings", "rust", "varpro_hip.rs")).read()
    assert re.search(r"pub fn vp_batch_create_fixed\(h: \*mut \*mut vp_batch, model: \*const vp_model_desc,", rust)
    assert re.search(r"fixed: \*const i32, values: \*const f64, per_problem: i32\) -> i32;", rust)
    assert re.search(r"pub fn vp_set_fixed_values\(h: \*mut vp_batch, values: \*const f64, per_problem: i32\) -> i32;", rust)
    cpp = open(os.path.join(ROOT, "varpro_amd", "cpp", "varpro.hpp")).read()
    assert "vp_batch_create_fixed(" in cpp and "vp_set_fixed_values(" in cpp and "void set_fixed_values(" in cpp
    # a null handle is refused by the library itself, without a device
    assert lib.vp_set_fixed_values(None, None, 0) == _lib.VP_ERR_INVALID
    assert lib.vp_batch_create_fixed(None, None, 0, 0, 0, 0, None, None, None, 0.0, 0, 0, None, None, None, 0) == _lib.VP_ERR_INVALID


def test_mask_and_values_from_the_dict():
    names = ["mu1", "s1", "mu2", "g2"]
    mask, free, held = fixed.fixed_mask(names, {"g2": 1.0, "s1": 2.0})
    assert mask.dtype == np.int32 and mask.tolist() == [0, 1, 0, 1] and free.tolist() == [0, 2] and held.tolist() == [1, 3]
    mask, free, held = fixed.fixed_mask(names, {})
    assert mask.tolist() == [0, 0, 0, 0] and held.size == 0
    for bad in ({"sigma": 1.0}, {n: 1.0 for n in names}, [("s1", 1.0)]):
        with pytest.raises(ValueError):
            fixed.fixed_mask(names, bad)
    v, per = fixed.fixed_values(names, {"g2": 1.5, "s1": np.float32(0.5)}, 3)
    assert not per and v.dtype == np.float64 and v.tolist() == [0.0, 0.5, 0.0, 1.5]
    v, per = fixed.fixed_values(names, {"g2": 1.5, "s1": np.array([1.0, 2.0, 3.0])}, 3)
    assert per and v.shape == (3, 4) and v[:, 1].tolist() == [1.0, 2.0, 3.0] and v[:, 3].tolist() == [1.5] * 3 and not v[:, [0, 2]].any()
    for bad in ({"s1": np.zeros(2)}, {"s1": np.zeros((3, 1))}):
        with pytest.raises(ValueError):
            fixed.fixed_values(names, bad, 3)


def test_expansion_to_full_order_and_the_scatter_of_the_covariance():
    free, held = np.array([0, 2]), np.array([1, 3])
    a_free = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    full = fixed.expand_columns(a_free, free, held, np.array([9.0, 0.5, 9.0, 1.5]), 4)
    assert np.array_equal(full, [[1.0, 0.5, 2.0, 1.5], [3.0, 0.5, 4.0, 1.5], [5.0, 0.5, 6.0, 1.5]])
    per = np.array([[0.0, 10.0, 0.0, 20.0], [0.0, 11.0, 0.0, 21.0], [0.0, 12.0, 0.0, 22.0]])
    full = fixed.expand_columns(a_free, free, held, per, 4)
    assert np.array_equal(full[:, held], per[:, held]) and np.array_equal(full[:, free], a_free)
    assert np.array_equal(fixed.reduce_columns(full, free), a_free) and fixed.reduce_columns(full, free).flags["C_CONTIGUOUS"]
    # fp32 handles read the values rounded to fp32
    f32 = fixed.expand_columns(a_free.astype(np.float32), free, held, np.array([0.0, 0.1, 0.0, 0.2]), 4)
    assert f32.dtype == np.float32 and f32[0, 1] == np.float32(0.1)
    # candidates (K, q) and (B, K, q) reduce along the last axis
    assert fixed.reduce_columns(np.arange(24.0).reshape(2, 3, 4), free).shape == (2, 3, 2)
    # statistics: [linear coefficients, nonlinear parameters], n = 2 -- rows and columns of fixed parameters exactly 0
    n = 2
    c = np.arange(1.0, 1.0 + 3 * 16).reshape(3, 4, 4)
    keep = np.concatenate([np.arange(n), n + free])
    cov = fixed.scatter_square(c, keep, n + 4)
    assert cov.shape == (3, 6, 6) and np.array_equal(cov[:, keep[:, None], keep[None, :]], c)
    for k in n + held:
        assert not cov[:, k, :].any() and not cov[:, :, k].any()
    ca = fixed.scatter_last(np.ones((3, 1, n, 2)), free, 4)
    assert ca.shape == (3, 1, n, 4) and (ca[..., free] == 1).all() and not ca[..., held].any()


class _Handle(fixed.FixedBatchProblem):
    """a FixedBatchProblem without a device handle: full-order arguments must be checked before the library is touched"""

    def __init__(self, B, names, fixed_dict):
        self.B, self.q_full = B, len(names)
        _mask, self.free, self.held = fixed.fixed_mask(names, fixed_dict)
        self.q = int(self.free.size)
        self._h = None

        class _NoLib:
            def __getattr__(self, name):
                raise AssertionError("the library was touched: %s" % name)
        self.lib = _NoLib()
        self.device_mode = False
        self.np_dtype = np.dtype(np.float64)
        self._fixed = dict(fixed_dict)


def test_full_order_arguments_are_checked_without_a_gpu():
    bp = _Handle(3, ["mu1", "s1", "mu2", "g2"], {"s1": 0.5, "g2": 1.0})
    assert np.array_equal(bp._reduce(np.array([1.0, 7.0, 2.0, 8.0])), [[1.0, 2.0]] * 3)
    assert np.array_equal(bp._reduce(np.arange(12.0).reshape(3, 4)), [[0.0, 2.0], [4.0, 6.0], [8.0, 10.0]])
    for bad in (np.zeros(2), np.zeros((3, 2)), np.zeros((2, 4))):
        with pytest.raises(ValueError):
            bp._reduce(bad)
    with pytest.raises(ValueError):
        bp.set_bounds(np.zeros(2), np.ones(2))          # reduced-order bounds: the mirror is in full order
    with pytest.raises(ValueError):
        bp.set_bounds([0.0, 0.0, 1.0, 0.0], [1.0, 1.0, 1.0, 1.0])  # lo == hi on a FREE parameter is still refused
    with pytest.raises(ValueError):
        bp.set_fixed(mu1=3.0)                           # not among the fixed parameters
    with pytest.raises(ValueError):
        bp.search(np.zeros((5, 2)))
    with pytest.raises(ValueError):
        vp.BatchProblem(vp.ExternalModel(2, 2, [(0, 0), (1, 1)]), np.zeros((2, 8)), fixed={"a": 1.0})


def test_dispatch_refuses_what_it_cannot_serve():
    class Mine(vp.BatchProblem):
        pass
    case, x, _alpha = fc.columns_case("e", 16)
    with pytest.raises(ValueError, match="FixedBatchProblem"):
        Mine(case.model(), np.zeros((2, 16)), fixed={"tau1": 1.0})   # a user's subclass has no full-order bookkeeping
    with pytest.raises(ValueError, match="fixed="):
        fixed.FixedBatchProblem(case.model(), np.zeros((2, 16)))     # ... and the subclass itself needs the dict
    with pytest.raises(ValueError, match="fixed="):
        fixed.FixedBatchProblem(case.model(), np.zeros((2, 16)), fixed=None)


def test_an_unfixed_problem_is_a_plain_batch_problem():
    assert vp.BatchProblem.__new__(vp.BatchProblem).__class__ is vp.BatchProblem
    assert vp.BatchProblem.__new__(vp.BatchProblem, None, None, fixed=None).__class__ is vp.BatchProblem
    assert vp.BatchProblem.__new__(vp.BatchProblem, None, None, fixed={}).__class__ is fixed.FixedBatchProblem
