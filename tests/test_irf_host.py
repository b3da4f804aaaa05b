"""CPU tier of the IRF reconvolution kinds (basis.EXP_DECAY_IRF, basis.IRF): what the Python layers accept and refuse
without a device, and the numpy reference of the GPU tier (tests/irf_cases.py) against the defining sums."""
import numpy as np
import pytest

import irf_cases as ic
import varpro_amd as vp
from varpro_amd import basis
from varpro_amd.model import check_irf, irf_columns, uniform_step


def test_builder_accepts_the_kinds_and_their_derivative():
    x = np.linspace(0.0, 25.0, 64)
    mdl = ic.lifetime_model(x)
    assert mdl.kinds == [basis.EXP_DECAY_IRF, basis.EXP_DECAY_IRF, basis.IRF, basis.CONST]
    assert mdl.param_indices == [(0,), (1,), (), ()] and mdl.pairs == [(0, 0, 0), (1, 0, 1)]
    d = mdl.desc()
    assert (d.n_basis, d.n_params) == (4, 2)
    assert list(d.kind)[:4] == [9, 9, 10, 0]
    assert [list(r) for r in d.param][:4] == [[0, -1], [1, -1], [-1, -1], [-1, -1]]
    assert basis.EXP_DECAY_IRF in basis.DEVICE_COLUMN and basis.IRF in basis.DEVICE_COLUMN
    # a mix with a peak kind and an older kind is one descriptor
    mix = (vp.SeparableModelBuilder(["tau", "mu", "s"]).function(["tau"], basis.EXP_DECAY_IRF).partial_deriv("tau")
           .function(["mu", "s"], basis.GAUSS).partial_deriv("mu").partial_deriv("s").invariant_function(basis.IRF)
           .independent_variable(x).initial_parameters([1.0, 3.0, 0.5]).build())
    assert mix.kinds == [9, 6, 10]


def test_builder_refuses_a_wrong_parameter_count():
    x = np.linspace(0.0, 1.0, 8)
    with pytest.raises(vp.ModelBuildError) as e:
        (vp.SeparableModelBuilder(["a", "b"]).function(["a", "b"], basis.EXP_DECAY_IRF).partial_deriv("a").partial_deriv("b")
         .independent_variable(x).initial_parameters([1.0, 2.0]).build())
    assert e.value.variant == "IncorrectParameterCount"
    with pytest.raises(vp.ModelBuildError) as e:  # the response takes no parameter
        (vp.SeparableModelBuilder(["a"]).function(["a"], basis.IRF).partial_deriv("a")
         .independent_variable(x).initial_parameters([1.0]).build())
    assert e.value.variant == "IncorrectParameterCount"
    with pytest.raises(vp.ModelBuildError) as e:  # ... and a decay is not invariant
        (vp.SeparableModelBuilder(["a"]).invariant_function(basis.EXP_DECAY_IRF)
         .independent_variable(x).initial_parameters([1.0]).build())
    assert e.value.variant == "IncorrectParameterCount"
    with pytest.raises(vp.ModelBuildError) as e:
        (vp.SeparableModelBuilder(["a"]).function(["a"], basis.EXP_DECAY_IRF)
         .independent_variable(x).initial_parameters([1.0]).build())
    assert e.value.variant == "MissingDerivative"


def test_builder_refuses_a_derivative_declared_on_the_response():
    x = np.linspace(0.0, 1.0, 8)
    with pytest.raises(vp.ModelBuildError) as e:
        (vp.SeparableModelBuilder(["a"]).function(["a"], basis.EXP_DECAY_IRF).partial_deriv("a")
         .invariant_function(basis.IRF).partial_deriv("a").independent_variable(x).initial_parameters([1.0]).build())
    assert e.value.variant == "IllegalCallToPartialDeriv"


def test_a_non_uniform_host_grid_is_refused():
    x = np.linspace(0.0, 25.0, 64)
    bad = x.copy()
    bad[17] += 2e-6 * (x[1] - x[0])
    assert uniform_step(x) == pytest.approx(25.0 / 63)
    assert uniform_step(np.array([3.0])) == 0.0            # m = 1 is allowed
    assert uniform_step(np.stack([x, 2 * x + 1])).shape == (2,)
    with pytest.raises(ValueError):
        uniform_step(bad)
    with pytest.raises(ValueError):
        uniform_step(np.stack([x, bad]))
    b = (vp.SeparableModelBuilder(["tau"]).function(["tau"], basis.EXP_DECAY_IRF).partial_deriv("tau")
         .independent_variable(bad).initial_parameters([1.0]))
    with pytest.raises(vp.ModelBuildError) as e:
        b.build()
    assert e.value.variant == "NonUniformGrid"
    # the same grid is fine for a model without these kinds
    (vp.SeparableModelBuilder(["tau"]).function(["tau"], basis.EXP_DECAY).partial_deriv("tau")
     .independent_variable(bad).initial_parameters([1.0]).build())
    # BatchProblem checks the grid it is given (a per-problem one included) before it creates anything
    mdl = ic.lifetime_model(x)
    with pytest.raises(ValueError) as e2:
        vp.BatchProblem(mdl, np.zeros((2, 64)), x=np.stack([x, bad]))
    assert "NonUniformGrid" in str(e2.value)


def test_a_response_of_the_wrong_length_or_shape_is_refused():
    B, m = 3, 64
    ok = np.ones(m)
    assert check_irf(ok, B, m)[1] is False and check_irf(np.ones((B, m)), B, m)[1] is True
    for bad in (np.ones(m + 1), np.ones((B, m - 1)), np.ones((B + 1, m)), np.ones((1, 1, m)), np.ones(())):
        with pytest.raises(ValueError) as e:
            check_irf(bad, B, m)
        assert "InvalidLengthOfIrf" in str(e.value)
    x = np.linspace(0.0, 25.0, m)
    mdl = ic.lifetime_model(x)
    with pytest.raises(ValueError) as e:
        vp.BatchProblem(mdl, np.zeros((B, m)), irf=np.ones(m + 1))
    assert "InvalidLengthOfIrf" in str(e.value)
    with pytest.raises(ValueError):  # a response for a model that has no use for it
        vp.BatchProblem(vp.multi_exponential_model(x, [1.0, 4.0]), np.zeros((B, m)), irf=ok)
    # the single-problem builder
    with pytest.raises(vp.SeparableProblemBuilderError) as e:
        vp.SeparableProblemBuilder.new(mdl).observations(np.zeros(m)).build()
    assert e.value.variant == "IrfMissing"
    with pytest.raises(vp.SeparableProblemBuilderError) as e:
        vp.SeparableProblemBuilder.new(mdl).observations(np.zeros(m)).instrument_response(np.ones(m - 2)).build()
    assert e.value.variant == "InvalidLengthOfIrf"
    with pytest.raises(vp.SeparableProblemBuilderError) as e:
        vp.SeparableProblemBuilder.new(mdl).observations(np.zeros(m)).instrument_response(np.ones((2, m))).build()
    assert e.value.variant == "InvalidLengthOfIrf"
    with pytest.raises(vp.SeparableProblemBuilderError) as e:
        (vp.SeparableProblemBuilder.new(vp.multi_exponential_model(x, [1.0, 4.0])).observations(np.zeros(m))
         .instrument_response(ok).build())
    assert e.value.variant == "UnexpectedIrf"


@pytest.mark.parametrize("tau_over_dt", [2.0, 37.5, 16000.0])
def test_the_sequential_recurrence_equals_the_direct_sums(tau_over_dt):
    """the reference of the GPU tier against the O(m^2) sums in long double at m = 37: every entry within a few units of
    eps (1 + l_i) |value| -- the sensitivity units of tests/test_gpu_irf.py (each step of the recurrence adds at most about
    one rounding of the running value, damped by rho)"""
    m = 37
    rng = np.random.default_rng(5)
    irf = ic.response(m) * rng.uniform(0.5, 1.5, m)
    dt = 0.21
    tau = tau_over_dt * dt
    F, H, D = ic.recurrence(irf, dt, tau)
    Fl, Hl, Gl, sc = ic.direct_sums(irf, dt, tau)
    assert H[0] == 0 and Hl[0] == 0 and F[0] == irf[0]
    eF, eD = ic.column_errors(F, D, irf, dt, tau, np.finfo(np.float64).eps)
    print("tau/dt = %g: recurrence against direct sums %.2f / %.2f units" % (tau_over_dt, eF, eD))
    assert eF <= 8 and eD <= 8
    assert np.abs(F.astype(ic.L) - Fl).max() <= 1e-13 * float(np.abs(Fl).max())
    assert np.abs(D.astype(ic.L) - sc * Hl).max() <= 1e-13 * float(np.abs(sc * Hl).max())
    # the identities the kernel's scan rests on: the affine map over s rows
    s = 5
    rho = np.exp(-ic.L(dt) / ic.L(tau))
    Floc, Hloc, _G, _sc = ic.direct_sums(irf[m - s:], dt, tau)
    assert abs(rho ** s * Fl[m - s - 1] + Floc[-1] - Fl[-1]) <= 1e-17 * abs(Fl[-1])
    assert abs(rho ** s * (Hl[m - s - 1] + s * Fl[m - s - 1]) + Hloc[-1] - Hl[-1]) <= 1e-17 * abs(Hl[-1])
    # the library's own host mirror is the same recurrence
    F2, D2 = irf_columns(irf, dt, tau)
    assert np.array_equal(F2, F) and np.allclose(D2, D, rtol=1e-15, atol=0)
    # fp32: the same code path in numpy float32
    F32, _H32, D32 = ic.recurrence(irf.astype(np.float32), np.float32(dt), np.float32(tau))
    assert F32.dtype == np.float32 and D32.dtype == np.float32
    e32 = ic.column_errors(F32, D32, irf.astype(np.float32), np.float32(dt), np.float32(tau), np.finfo(np.float32).eps)
    assert max(e32) <= 8


def test_host_mirror_of_the_model_surface():
    """SeparableModel.eval / eval_partial_deriv of a model with these kinds run on the host, with the model's response"""
    m = 50
    x = np.linspace(0.0, 25.0, m)
    irf = ic.response(m)
    mdl = ic.lifetime_model(x)
    with pytest.raises(vp.ModelError):
        mdl.eval()
    mdl.irf = irf
    P = mdl.eval()
    assert P.shape == (m, 4)
    assert np.array_equal(P, ic.lifetime_columns(irf, ic.grid_step(x), [1.0, 4.0]))
    assert np.allclose(mdl.eval_partial_deriv(1)[:, 1], ic.recurrence(irf, ic.grid_step(x), 4.0)[2], rtol=1e-15, atol=0)
    assert not mdl.eval_partial_deriv(1)[:, [0, 2, 3]].any()
