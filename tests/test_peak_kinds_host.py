"""CPU tier of the peak / baseline basis kinds (VP_BASIS_GAUSS, VP_BASIS_LORENTZ, VP_BASIS_LINEAR): constants, builder and
the numpy mirror of the column kernel.  The formulas are the closures `gauss*` / `lorentz*` of tests/test_gpu_external.py,
which also drive the checker of the GPU tier (tests/test_gpu_peak_kinds.py)."""
import os
import re

import numpy as np
import pytest

import varpro_amd as vp
from varpro_amd import _lib, basis
from test_gpu_external import gauss, gauss_dmu, gauss_dsg, lorentz, lorentz_dga, lorentz_dmu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def peak_model(x, a0=(3.0, 0.7, 6.4, 0.9), dtype=np.float64):
    """c1 Gauss(mu1, s1) + c2 Lorentz(mu2, g2) + c3 t + c4: n = 4, q = 4, p = 4"""
    return (vp.SeparableModelBuilder(["mu1", "s1", "mu2", "g2"], dtype=dtype)
            .function(["mu1", "s1"], basis.GAUSS).partial_deriv("mu1").partial_deriv("s1")
            .function(["mu2", "g2"], basis.LORENTZ).partial_deriv("mu2").partial_deriv("g2")
            .invariant_function(basis.LINEAR)
            .invariant_function(basis.CONST)
            .independent_variable(x).initial_parameters(list(a0)).build())


def test_kinds_match_the_header():
    header = open(os.path.join(ROOT, "include", "varpro_hip.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\bVP_BASIS_([A-Z_]+) = (\d+)", header))
    assert (enum["GAUSS"], enum["LORENTZ"], enum["LINEAR"]) == (6, 7, 8)
    assert (basis.GAUSS, basis.LORENTZ, basis.LINEAR) == (6, 7, 8)
    assert (_lib.VP_BASIS_GAUSS, _lib.VP_BASIS_LORENTZ, _lib.VP_BASIS_LINEAR) == (6, 7, 8)
    for name in ("CONST", "EXP_DECAY", "EXP_RATE", "EXP_COS", "SIN_PHASE", "GAUSS", "LORENTZ", "LINEAR"):
        assert getattr(basis, name) == enum[name] == getattr(_lib, "VP_BASIS_" + name)
    assert (basis.ARITY[basis.GAUSS], basis.ARITY[basis.LORENTZ], basis.ARITY[basis.LINEAR]) == (2, 2, 0)
    assert set(basis.NAME) == set(basis.ARITY)
    # the other mirrors of the header
    rust = open(os.path.join(ROOT, "bindings", "rust", "varpro_hip.rs")).read()
    for name, val in (("GAUSS", 6), ("LORENTZ", 7), ("LINEAR", 8)):
        assert re.search(r"VP_BASIS_%s: i32 = %d;" % (name, val), rust)
    cpp = open(os.path.join(ROOT, "varpro_amd", "cpp", "varpro.hpp")).read()
    for name in ("GAUSS", "LORENTZ", "LINEAR"):
        assert "VP_BASIS_" + name in cpp


def test_builder_accepts_the_kinds_and_reports_the_existing_errors():
    x = np.linspace(0.0, 10.0, 32)
    mdl = peak_model(x)
    assert (mdl.parameter_count(), mdl.base_function_count(), mdl.output_len()) == (4, 4, 32)
    assert mdl.pairs == [(0, 0, 0), (0, 1, 1), (1, 0, 2), (1, 1, 3)]
    with pytest.raises(vp.ModelBuildError) as e:  # a Gaussian takes two parameters
        vp.SeparableModelBuilder(["mu"]).function(["mu"], basis.GAUSS).build()
    assert e.value.variant == "IncorrectParameterCount"
    with pytest.raises(vp.ModelBuildError) as e:
        vp.SeparableModelBuilder(["a", "b", "c"]).function(["a", "b", "c"], basis.LORENTZ).build()
    assert e.value.variant == "IncorrectParameterCount"
    with pytest.raises(vp.ModelBuildError) as e:  # the linear baseline is invariant
        vp.SeparableModelBuilder(["a"]).function(["a"], basis.LINEAR).build()
    assert e.value.variant == "IncorrectParameterCount"
    with pytest.raises(vp.ModelBuildError) as e:
        vp.SeparableModelBuilder(["mu", "s"]).invariant_function(basis.GAUSS).build()
    assert e.value.variant == "IncorrectParameterCount"
    with pytest.raises(vp.ModelBuildError) as e:
        (vp.SeparableModelBuilder(["mu", "s"]).function(["mu", "s"], basis.GAUSS).partial_deriv("mu")
         .independent_variable(x).initial_parameters([1.0, 1.0]).build())
    assert e.value.variant == "MissingDerivative"


def test_descriptor_carries_kinds_and_parameter_table():
    d = peak_model(np.linspace(0.0, 1.0, 8)).desc()
    assert (d.n_basis, d.n_params) == (4, 4)
    assert list(d.kind)[:4] == [basis.GAUSS, basis.LORENTZ, basis.LINEAR, basis.CONST]
    assert [list(r) for r in d.param][:4] == [[0, 1], [2, 3], [-1, -1], [-1, -1]]
    assert all(list(r) == [-1, -1] for r in list(d.param)[4:])


@pytest.mark.parametrize("m", [17, 1000])
def test_eval_and_partial_derivatives_equal_the_closures(m):
    """SeparableModel.eval / eval_partial_deriv of Gauss + Lorentz + linear + const on the host: the closures to 1e-15"""
    rng = np.random.default_rng(m)
    x = np.linspace(0.0, 10.0, m)
    for _ in range(4):
        mu1, s1, mu2, g2 = rng.uniform(2.5, 3.5), rng.uniform(0.4, 0.9), rng.uniform(6.0, 7.0), rng.uniform(0.5, 1.2)
        mdl = peak_model(x, (mu1, s1, mu2, g2))
        Phi = mdl.eval()
        ref = np.stack([gauss(x, mu1, s1), lorentz(x, mu2, g2), x, np.ones_like(x)], 1)
        assert Phi.shape == (m, 4)
        assert np.abs(Phi - ref).max() <= 1e-15 * np.abs(ref).max()
        assert (np.abs(Phi - ref) <= 1e-15 * np.abs(ref)).all()
        cols = {0: (0, gauss_dmu(x, mu1, s1)), 1: (0, gauss_dsg(x, mu1, s1)), 2: (1, lorentz_dmu(x, mu2, g2)),
                3: (1, lorentz_dga(x, mu2, g2))}
        for k, (j, col) in cols.items():
            D = mdl.eval_partial_deriv(k)
            want = np.zeros((m, 4))
            want[:, j] = col
            assert (np.abs(D - want) <= 1e-15 * np.abs(want)).all(), k
    with pytest.raises(vp.ModelError):
        mdl.eval_partial_deriv(4)
    # a model that mixes a peak with the older kinds is mirrored on the host as well
    mix = (vp.SeparableModelBuilder(["mu", "s", "tau"])
           .function(["mu", "s"], basis.GAUSS).partial_deriv("mu").partial_deriv("s")
           .function(["tau"], basis.EXP_DECAY).partial_deriv("tau")
           .invariant_function(basis.LINEAR).invariant_function()
           .independent_variable(x).initial_parameters([3.0, 0.5, 2.0]).build())
    Phi = mix.eval()
    assert np.abs(Phi[:, 1] - np.exp(-x / 2.0)).max() <= 1e-15 and np.array_equal(Phi[:, 2], x)
    assert np.abs(mix.eval_partial_deriv(2)[:, 1] - np.exp(-x / 2.0) * x / 4.0).max() <= 1e-15
