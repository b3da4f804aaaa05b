"""CPU tier of the periodic IRF reconvolution kind (basis.EXP_DECAY_IRF_PERIODIC): what the Python layers and the library
refuse without a device, and the numpy mirror (varpro_amd.model.irf_columns with a period) against the long-double
reference of tests/irf_periodic_cases.py."""
import ctypes as C

import numpy as np
import pytest

import irf_cases as ic
import irf_periodic_cases as pc
import varpro_amd as vp
from varpro_amd import _lib, basis
from varpro_amd.model import irf_columns

EPS64 = float(np.finfo(np.float64).eps)
RATIOS = np.geomspace(2.0, 16000.0, 6)  # tau/dt


def test_builder_accepts_the_kind_with_one_parameter():
    x = np.linspace(0.0, 12.5, 64)
    mdl = pc.periodic_lifetime_model(x)
    assert basis.EXP_DECAY_IRF_PERIODIC == 11 == _lib.VP_BASIS_EXP_DECAY_IRF_PERIODIC
    assert mdl.kinds == [11, 11, basis.IRF, basis.CONST] and mdl.pairs == [(0, 0, 0), (1, 0, 1)]
    assert list(mdl.desc().kind)[:4] == [11, 11, 10, 0]
    assert basis.EXP_DECAY_IRF_PERIODIC in basis.IRF_KINDS and basis.EXP_DECAY_IRF_PERIODIC in basis.DEVICE_COLUMN
    assert basis.ARITY[11] == 1 and basis.NAME[11] == "exp_decay_irf_periodic"
    # kinds 9, 10 and 11 in one descriptor
    mix = (vp.SeparableModelBuilder(["a", "b"]).function(["a"], basis.EXP_DECAY_IRF).partial_deriv("a")
           .function(["b"], basis.EXP_DECAY_IRF_PERIODIC).partial_deriv("b").invariant_function(basis.IRF)
           .independent_variable(x).initial_parameters([1.0, 2.0]).build())
    assert mix.kinds == [9, 11, 10]
    with pytest.raises(vp.ModelBuildError) as e:
        (vp.SeparableModelBuilder(["a", "b"]).function(["a", "b"], basis.EXP_DECAY_IRF_PERIODIC).partial_deriv("a")
         .partial_deriv("b").independent_variable(x).initial_parameters([1.0, 2.0]).build())
    assert e.value.variant == "IncorrectParameterCount"


def test_builder_refuses_a_non_uniform_grid():
    x = np.linspace(0.0, 12.5, 64)
    x[17] += 2e-6 * (x[1] - x[0])
    with pytest.raises(vp.ModelBuildError) as e:
        (vp.SeparableModelBuilder(["tau"]).function(["tau"], basis.EXP_DECAY_IRF_PERIODIC).partial_deriv("tau")
         .independent_variable(x).initial_parameters([1.0]).build())
    assert e.value.variant == "NonUniformGrid"


def test_irf_period_is_validated_without_a_device():
    B, m = 3, 64
    x = np.linspace(0.0, 12.5, m)
    dt = x[1] - x[0]
    mdl = pc.periodic_lifetime_model(x)
    Y = np.zeros((B, m))
    for bad in (float("nan"), -1.0, 0.99 * m * dt, (1 - 2e-6) * m * dt):
        with pytest.raises(ValueError) as e:
            vp.BatchProblem(mdl, Y, irf_period=bad)
        assert "InvalidIrfPeriod" in str(e.value), bad
    # per-problem grids: the longest record decides
    X = np.stack([x, 2 * x, x])
    with pytest.raises(ValueError) as e:
        vp.BatchProblem(mdl, Y, x=X, irf_period=1.5 * m * dt)
    assert "InvalidIrfPeriod" in str(e.value)
    with pytest.raises(ValueError) as e:  # a model without the periodic kind
        vp.BatchProblem(ic.lifetime_model(x), Y, irf_period=2 * m * dt)
    assert "EXP_DECAY_IRF_PERIODIC" in str(e.value)
    # the single-problem builder
    with pytest.raises(vp.SeparableProblemBuilderError) as e:
        (vp.SeparableProblemBuilder.new(mdl).observations(np.zeros(m)).instrument_response(np.ones(m), period=0.5 * m * dt)
         .build())
    assert e.value.variant == "InvalidIrfPeriod"
    with pytest.raises(vp.SeparableProblemBuilderError) as e:
        (vp.SeparableProblemBuilder.new(ic.lifetime_model(x)).observations(np.zeros(m))
         .instrument_response(np.ones(m), period=2 * m * dt).build())
    assert e.value.variant == "UnexpectedIrfPeriod"


def test_the_library_refuses_a_null_handle():
    lib = _lib.load()
    assert "vp_set_irf_period" in _lib.ABI_SYMBOLS
    assert lib.vp_set_irf_period(None, C.c_double(1.0)) == _lib.VP_ERR_INVALID


def test_the_long_double_reference_equals_a_brute_force_sum_over_periods():
    """m = 12, the closed-form series per pair against the defining sum over 60 periods (rho^(60 P) is far below rounding)"""
    m, dt = 12, 0.21
    irf = ic.response(m) * np.random.default_rng(2).uniform(0.5, 1.5, m)
    for tau_over_dt in (2.0, 9.0):
        for period in (None, (1.37 * m + 0.5) * dt):
            tau = tau_over_dt * dt
            Fl, Hl, _Gl, _sc = pc.periodic_sums(irf, dt, tau, period)
            Fb, Hb = pc.brute_force_sums(irf, dt, tau, period)
            assert np.abs(Fl - Fb).max() <= 1e-17 * np.abs(Fb).max() and np.abs(Hl - Hb).max() <= 1e-17 * np.abs(Hb).max()
    # the second-moment sum: a central difference of H in rho (d/dln rho of sum d rho^d = sum d^2 rho^d)
    tau, h = 5.0 * dt, 1e-5
    up, dn = (pc.periodic_sums(irf, dt * (1 + s * h), tau, None)[1] for s in (1, -1))
    Gl = pc.periodic_sums(irf, dt, tau, None)[2]
    assert np.abs((dn - up) / (2 * h) * (tau / dt) - Gl).max() <= 1e-8 * np.abs(Gl).max()


@pytest.mark.parametrize("longer", [False, True])
@pytest.mark.parametrize("m", [2, 127, 129, 1030])
def test_numpy_mirror_against_long_double(m, longer):
    """fp64, the default period and period = (1.37 m + 0.5) dt, tau/dt from 2 to 16 000: errors in the sensitivity units of
    irf_cases.column_errors with l_i = H_i/F_i of the periodic sums.  Measured: at most 0.9 units; the limit is 2."""
    dt = 0.02
    irf = ic.response(m) * np.random.default_rng(m).uniform(0.5, 1.5, m)
    period = (1.37 * m + 0.5) * dt if longer else None
    worst = 0.0
    for ratio in RATIOS:
        tau = ratio * dt
        F, D = pc.mirror(irf, dt, tau, period)
        worst = max(worst, *pc.column_errors(F, D, irf, dt, tau, EPS64, period))
    print("mirror m=%d longer=%s: %.3f units" % (m, longer, worst))
    assert worst <= 2


def test_long_period_limit_is_the_zero_start_recurrence_bit_for_bit():
    m, dt = 129, 0.02
    irf = ic.response(m)
    for ratio in RATIOS:
        tau = ratio * dt
        F0, D0 = irf_columns(irf, dt, tau)
        F1, D1 = irf_columns(irf, dt, tau, period=1e4 * tau)
        assert np.array_equal(F0, F1) and np.array_equal(D0, D1)
    F32, D32 = irf_columns(irf.astype(np.float32), np.float32(dt), np.float32(0.5))
    G32, E32 = irf_columns(irf.astype(np.float32), np.float32(dt), np.float32(0.5), period=200.0)  # exp(-400) == 0 in fp32
    assert np.array_equal(F32, G32) and np.array_equal(D32, E32)


@pytest.mark.parametrize("m", [16, 129])
def test_one_period_per_record_is_a_circular_convolution(m):
    """P = m: Phi = irf (*) rho^s / (1 - rho^m), s = 0..m-1, circularly, in long double; and the column of a cyclically
    shifted response is the cyclically shifted column -- both to the rule of the mirror test"""
    dt = 0.02
    irf = ic.response(m) * np.random.default_rng(7 + m).uniform(0.5, 1.5, m)
    for ratio in RATIOS:
        tau = ratio * dt
        sums = pc.periodic_sums(irf, dt, tau)
        rho = np.exp(-(ic.L(dt) / ic.L(tau)))
        kern = rho ** np.arange(m).astype(ic.L) / (1 - rho ** m)
        circ = np.array([sum(irf[k].astype(ic.L) * kern[(i - k) % m] for k in range(m)) for i in range(m)])
        lF = sums[1] / sums[0]
        F, D = pc.mirror(irf, dt, tau)
        assert ic.unit_errors(F, circ, lF, EPS64) <= 2
        Fr, Dr = pc.mirror(np.roll(irf, 5), dt, tau)
        assert ic.unit_errors(Fr, np.roll(sums[0], 5), np.roll(lF, 5), EPS64) <= 2
        assert ic.unit_errors(Dr, np.roll(sums[3] * sums[1], 5), np.roll(sums[2] / sums[1], 5), EPS64) <= 2


def test_host_mirror_of_the_model_surface():
    m = 50
    x = np.linspace(0.0, 12.5, m)
    irf = ic.response(m)
    mdl = pc.periodic_lifetime_model(x)
    mdl.irf = irf
    dt = ic.grid_step(x)
    assert np.array_equal(mdl.eval(), pc.periodic_lifetime_columns(irf, dt, [1.0, 4.0]))
    mdl.irf_period = 1.3 * m * dt
    P = mdl.eval()
    assert np.allclose(P, pc.periodic_lifetime_columns(irf, dt, [1.0, 4.0], 1.3 * m * dt), rtol=1e-14, atol=0)
    assert np.allclose(mdl.eval_partial_deriv(1)[:, 1], pc.mirror(irf, dt, 4.0, 1.3 * m * dt)[1], rtol=1e-14, atol=0)
