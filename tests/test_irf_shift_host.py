"""CPU tier of the shifted IRF kinds (basis.EXP_DECAY_IRF_SHIFT, IRF_SHIFT, EXP_DECAY_IRF_PERIODIC_SHIFT): the numpy mirror
of the resample kernel (varpro_amd.model.irf_shifted) against the long-double definition of tests/irf_shift_cases.py, the
properties the convention promises (include/varpro_hip.h, "Shifted IRF reconvolution"), the builder's rules and the constants
of the four language surfaces."""
import os
import re

import numpy as np
import pytest

import irf_cases as ic
import irf_shift_cases as sh
import varpro_amd as vp
from varpro_amd import _lib, basis
from varpro_amd.model import irf_columns, irf_shifted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = {np.float64: float(np.finfo(np.float64).eps), np.float32: float(np.finfo(np.float32).eps)}
SHIFTS = (0.0, 0.37, -2.6, 3.0, 1e-20, -1e-20, 17.25, -40.5)  # bins


def _response(m, dtype=np.float64):
    return (ic.response(m, 0.3, 0.04) * np.random.default_rng(m).uniform(0.5, 1.5, m)).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("m", [2, 5, 129, 1030])
def test_mirror_against_the_long_double_definition(m, dtype):
    """errors in units of eps (1 + |s|) sum_a |w_a| |tap| (over dt for g').  The limit, reasoned: a weight is a cubic with
    coefficients up to 5 (9 for w') in Horner form, three or four roundings of intermediates no larger than 5 (10): at most
    about 3 eps absolute each, 10 eps over the four; the taps of one stencil of this response lie within a factor 3 of each
    other (the jitter of 0.5 .. 1.5), so that is at most 30 units where the smallest tap carries the unit; the four-term
    sum and the division add 4, the rounding of s = delta/dt, eps |s| / 2 bins, stays below the factor (1 + |s|): 32 + 4."""
    T = dtype
    dt = T(5.0 / 256)  # (a short mantissa: an integer number of bins is an exact delta and an exact quotient delta/dt,
    # so the reference and the mirror take the same stencil there)
    irf = _response(m, dtype)
    worst = 0.0
    for s in SHIFTS:
        delta = T(s) * dt
        g, dg = irf_shifted(irf, dt, delta)
        assert g.dtype == dtype and dg.dtype == dtype and g.shape == (m,)
        worst = max(worst, *sh.shift_errors(g, dg, irf, dt, delta, EPS[dtype]))
    print("mirror %s m=%d: %.3f units" % (np.dtype(dtype).name, m, worst))
    assert worst <= 36


def test_weights_sum_to_one_and_their_derivatives_to_zero():
    for f in np.linspace(0.0, 1.0, 41).astype(sh.L):
        w, d = sh.weights(f)
        assert abs(sum(w) - 1) <= 1e-18 and abs(sum(d)) <= 1e-18
    w, d = sh.weights(sh.L(0))
    assert w == [0, 1, 0, 0]


def test_derivative_against_a_central_difference():
    m, dt = 129, 0.02
    irf = _response(m)
    for s in (0.37, -2.6, 0.5, 0.999):  # (inside one piece of the cubic: across a knot g'' jumps, the next test's subject)
        h = 1e-6 * dt
        up, dn = irf_shifted(irf, dt, s * dt + h)[0], irf_shifted(irf, dt, s * dt - h)[0]
        dg = irf_shifted(irf, dt, s * dt)[1]
        assert np.abs((up - dn) / (2 * h) - dg).max() <= 1e-6 * np.abs(dg).max()


@pytest.mark.parametrize("s0", [1, -1, 2, -2])
def test_derivative_is_continuous_across_integer_shifts(s0):
    m, dt = 129, 0.02
    irf = _response(m)
    lo, hi = irf_shifted(irf, dt, (s0 - 1e-9) * dt)[1], irf_shifted(irf, dt, (s0 + 1e-9) * dt)[1]
    assert np.abs(hi - lo).max() <= 1e-7 * np.abs(hi).max()  # (|g''| 2e-9 bins: the cubic is C1, not C2)
    glo, ghi = irf_shifted(irf, dt, (s0 - 1e-9) * dt)[0], irf_shifted(irf, dt, (s0 + 1e-9) * dt)[0]
    assert np.abs(ghi - glo).max() <= 1e-7 * np.abs(ghi).max()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_zero_shift_is_the_response_bit_for_bit_and_integer_shifts_move_the_rows(dtype):
    m = 37
    x = (0.25 * np.arange(m)).astype(dtype)  # dt a power of two: delta / dt is exact
    dt = ic.grid_step(x)
    irf = _response(m, dtype)
    assert np.array_equal(irf_shifted(irf, dt, 0.0)[0], irf)
    assert np.array_equal(irf_shifted(irf, dt, -0.0)[0], irf)
    for k in (1, 3, -2, -7, m - 1, -(m - 1)):
        g = irf_shifted(irf, dt, dtype(0.25 * k))[0]
        want = np.zeros(m, dtype)
        if k > 0:
            want[k:] = irf[:m - k]
        else:
            want[:m + k] = irf[-k:]
        assert np.array_equal(g, want), k


def test_shifts_beyond_the_record_give_zeros_and_non_finite_shifts_nan():
    m, dt = 16, 0.5
    irf = _response(m)
    for s in (m + 2, -(m + 2), m + 5, 1e30, -1e300):
        g, dg = irf_shifted(irf, dt, s * dt)
        assert (g == 0).all() and (dg == 0).all()
    for s in (m + 1.5, -(m + 1.5)):  # the taps have left the record already
        g, dg = irf_shifted(irf, dt, s * dt)
        assert (g == 0).all() and (dg == 0).all()
    for bad in (np.nan, np.inf, -np.inf):
        g, dg = irf_shifted(irf, dt, bad)
        assert np.isnan(g).all() and np.isnan(dg).all()


def test_builder_rules():
    x = np.linspace(0.0, 25.0, 64)
    mdl = sh.shifted_model(x, scatter=True)
    assert mdl.kinds == [12, 12, 13, 0]
    assert mdl.pairs == [(0, 0, 0), (0, 1, 2), (1, 0, 1), (1, 1, 2), (2, 0, 2)]
    assert list(mdl.desc().kind)[:4] == [12, 12, 13, 0] and list(mdl.desc().param[2]) == [2, -1]
    per = sh.shifted_model(x, kind=basis.EXP_DECAY_IRF_PERIODIC_SHIFT)
    assert per.kinds == [14, 14, 0] and len(per.pairs) == 4

    def build(b):
        return b.independent_variable(x).initial_parameters([1.0, 2.0, 0.0]).build()

    # arity
    with pytest.raises(vp.ModelBuildError) as e:
        build(vp.SeparableModelBuilder(["a", "b", "d"]).function(["a"], basis.EXP_DECAY_IRF_SHIFT).partial_deriv("a"))
    assert e.value.variant == "IncorrectParameterCount"
    with pytest.raises(vp.ModelBuildError) as e:
        build(vp.SeparableModelBuilder(["a", "b", "d"]).function(["a", "d"], basis.IRF_SHIFT).partial_deriv("a").partial_deriv("d"))
    assert e.value.variant == "IncorrectParameterCount"
    # both derivatives must be declared
    with pytest.raises(vp.ModelBuildError) as e:
        build(vp.SeparableModelBuilder(["a", "b", "d"]).function(["a", "d"], basis.EXP_DECAY_IRF_SHIFT).partial_deriv("a")
              .function(["b", "d"], basis.EXP_DECAY_IRF_SHIFT).partial_deriv("b").partial_deriv("d"))
    assert e.value.variant == "MissingDerivative"
    # one delta
    with pytest.raises(vp.ModelBuildError) as e:
        build(vp.SeparableModelBuilder(["a", "b", "d"]).function(["a", "b"], basis.EXP_DECAY_IRF_SHIFT).partial_deriv("a")
              .partial_deriv("b").function(["d"], basis.IRF_SHIFT).partial_deriv("d"))
    assert e.value.variant == "SeveralIrfShifts" and "irf_shift" in str(e.value)
    # delta is not shared with a function of another kind, nor with a tau
    with pytest.raises(vp.ModelBuildError) as e:
        build(vp.SeparableModelBuilder(["a", "b", "d"]).function(["a", "d"], basis.EXP_DECAY_IRF_SHIFT).partial_deriv("a")
              .partial_deriv("d").function(["b"], basis.EXP_DECAY_IRF).partial_deriv("b").function(["d"], basis.EXP_DECAY)
              .partial_deriv("d"))
    assert e.value.variant == "IrfShiftShared" and "exp_decay" in str(e.value)
    with pytest.raises(vp.ModelBuildError) as e:
        build(vp.SeparableModelBuilder(["a", "b", "d"]).function(["a", "d"], basis.EXP_DECAY_IRF_SHIFT).partial_deriv("a")
              .partial_deriv("d").function(["d", "b"], basis.EXP_DECAY_IRF_SHIFT).partial_deriv("d").partial_deriv("b"))
    assert e.value.variant in ("SeveralIrfShifts", "IrfShiftShared")
    # kinds 9 - 11 next to 12 - 14
    mix = build(vp.SeparableModelBuilder(["a", "b", "d"]).function(["a", "d"], basis.EXP_DECAY_IRF_SHIFT).partial_deriv("a")
                .partial_deriv("d").function(["b"], basis.EXP_DECAY_IRF).partial_deriv("b").invariant_function(basis.IRF))
    assert mix.kinds == [12, 9, 10]


def test_host_mirror_of_the_model_surface():
    m = 50
    x = np.linspace(0.0, 25.0, m)
    irf = ic.response(m, 0.2, 0.05)
    dt = ic.grid_step(x)
    for kind in (basis.EXP_DECAY_IRF_SHIFT, basis.EXP_DECAY_IRF_PERIODIC_SHIFT):
        mdl = sh.shifted_model(x, kind=kind, scatter=True)
        mdl.irf = irf
        a = np.array([1.0, 4.0, 0.4 * dt])
        mdl.set_params(a)
        assert np.array_equal(mdl.eval(), sh.model_columns(irf, dt, a, kind, scatter=True))
        g, dg = irf_shifted(irf, dt, a[2])
        per = 0.0 if kind == basis.EXP_DECAY_IRF_PERIODIC_SHIFT else None
        d = mdl.eval_partial_deriv(2)
        assert np.array_equal(d[:, 0], irf_columns(dg, dt, 1.0, per)[0]) and np.array_equal(d[:, 2], dg) and (d[:, 3] == 0).all()
        assert np.array_equal(mdl.eval_partial_deriv(1)[:, 1], irf_columns(g, dt, 4.0, per)[1])


def test_constants_agree_in_the_header_python_cpp_and_rust():
    want = {"VP_BASIS_EXP_DECAY_IRF_SHIFT": 12, "VP_BASIS_IRF_SHIFT": 13, "VP_BASIS_EXP_DECAY_IRF_PERIODIC_SHIFT": 14}
    assert (basis.EXP_DECAY_IRF_SHIFT, basis.IRF_SHIFT, basis.EXP_DECAY_IRF_PERIODIC_SHIFT) == (12, 13, 14)
    assert [basis.ARITY[k] for k in (12, 13, 14)] == [2, 1, 2]
    assert [basis.NAME[k] for k in (12, 13, 14)] == ["exp_decay_irf_shift", "irf_shift", "exp_decay_irf_periodic_shift"]
    for k in (12, 13, 14):
        assert k in basis.IRF_KINDS and k in basis.DEVICE_COLUMN
    header = open(os.path.join(ROOT, "include", "varpro_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "varpro_hip.rs")).read()
    cpp = open(os.path.join(ROOT, "varpro_amd", "cpp", "varpro.hpp")).read()
    for name, value in want.items():
        assert getattr(_lib, name) == value
        assert re.search(r"\b%s = %d\b" % (name, value), header), name
        assert re.search(r"pub const %s: i32 = %d;" % (name, value), rust), name
    for cname, name in (("ExpDecayIrfShift", "VP_BASIS_EXP_DECAY_IRF_SHIFT"), ("IrfShift", "VP_BASIS_IRF_SHIFT"),
                        ("ExpDecayIrfPeriodicShift", "VP_BASIS_EXP_DECAY_IRF_PERIODIC_SHIFT")):
        assert re.search(r"\b%s = %s\b" % (cname, name), cpp), cname
    assert "Shifted IRF reconvolution" in header
