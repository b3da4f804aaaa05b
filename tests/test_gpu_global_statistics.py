"""GPU tier: fit statistics of global fits (vp_global_statistics / BatchProblem.global_statistics /
LevMarSolver.fit_with_global_statistics) -- S = 1 against vp_statistics, small global fits against the oracle's
FitStatistics of the stacked problem, large S and every route against the block formulas of
test_global_statistics_math.py, refusals and status 4, and a calibration that does not depend on the derivation."""
import ctypes

import numpy as np
import pytest

import refdata as rd
import varpro_amd as vp
from models import double_exp_builder_model, oleary_model
from oracle import oracle as O
from test_global_statistics_math import MODELS, _rel, block_stats, oracle_stacked_stats, split
from varpro_amd import _lib, basis, synth
from varpro_amd.model import SeparableModel

pytestmark = pytest.mark.gpu


def desc_columns(mdl, x, alpha):
    """UNweighted Phi (n, m) and dPhi (P, m) of a descriptor model from the oracle, pairs in vp_basis order"""
    d = mdl.desc()
    pb, pp = [], []
    for j in range(d.n_basis):
        for k in range(2):
            if d.param[j][k] >= 0:
                pb.append(j)
                pp.append(d.param[j][k])
    Phi = O.eval_phi(mdl, x, alpha)
    D = {k: O.eval_dphi(mdl, x, alpha, k) for k in set(pp)}
    dPhi = np.stack([D[pp[p]][pb[p]] for p in range(len(pb))]) if pb else np.zeros((0, x.size))
    return Phi, dPhi, pb, pp


def generic_model(x):
    kinds = [basis.EXP_DECAY, basis.EXP_RATE, basis.EXP_COS, basis.CONST]
    params = [(0,), (1,), (2, 3), ()]
    alpha = np.array([1.7, 0.9, 0.25, 1.3])
    return SeparableModel(["a", "b", "c", "d"], kinds, params, x, alpha), alpha


def two_exp_model(x, initial):  # n = 2, q = 2: no constant
    return (vp.SeparableModelBuilder(["t1", "t2"]).initial_parameters(initial)
            .function(["t1"], basis.EXP_DECAY).partial_deriv("t1")
            .function(["t2"], basis.EXP_DECAY).partial_deriv("t2").independent_variable(x).build())


def global_data(rng, mdl, x, alpha, S, noise):
    Phi = O.eval_phi(mdl, x, alpha)
    Ct = rng.uniform(1.0, 5.0, (S, Phi.shape[0]))
    return Ct @ Phi + noise * rng.standard_normal((S, x.size))


def check_against_blocks(g, b, Phi, dPhi, pb, pp, q, w, C, Y, tol, band_rhs=None):
    ref = block_stats(Phi, dPhi, pb, pp, q, w, C, Y, band_rhs=band_rhs)
    assert int(g["status"][b]) == 0
    assert abs(g["reduced_chi2"][b] - ref["chi2"]) <= tol * ref["chi2"]
    assert _rel(g["cov_alpha"][b], ref["cov_alpha"]) <= tol
    assert _rel(g["coef_cov"][b], ref["coef_cov"]) <= tol
    assert _rel(g["coef_alpha_cov"][b], ref["coef_alpha_cov"]) <= tol
    if g["conf_sigma"] is not None:
        band = g["conf_sigma"][b] if band_rhs is None else g["conf_sigma"][b][band_rhs]
        assert _rel(band, ref["band"]) <= tol
    assert g["dof"] == ref["dof"]


# ---- 1. S = 1: vp_global_statistics == vp_statistics (the (n+q)^2 matrix re-ordered into blocks) ----
def _s1_cases():
    d = synth.double_exp_batch(16, m=1024, noise=1e-3)
    w = np.linspace(0.5, 2.0, 1024)
    yield "double_exp", double_exp_builder_model(d["x"], d["tau_guess"][0]), d["x"], d["Y"], d["tau_guess"], w
    yield ("oleary", oleary_model(rd.OLEARY_T, rd.OLEARY_GUESS), rd.OLEARY_T, rd.OLEARY_Y[None], rd.OLEARY_GUESS[None],
           rd.OLEARY_W)
    x = 8.0 * np.arange(600) / 599 + 0.05
    mdl, alpha = generic_model(x)
    rng = np.random.default_rng(4)
    Y = np.concatenate([global_data(rng, mdl, x, alpha, 1, 1e-3) for _ in range(3)])
    yield "generic", mdl, x, Y, np.tile(alpha * 1.02, (3, 1)), np.linspace(0.5, 2.0, 600)


@pytest.mark.parametrize("case", ["double_exp", "oleary", "generic"])
def test_single_rhs_equals_vp_statistics(case):
    name, mdl, x, Y, guess, w = next(c for c in _s1_cases() if c[0] == case)
    bp = vp.BatchProblem(mdl, Y, x=x, weights=w)
    bp.fit(guess)
    st = bp.statistics(want_confidence_sigma=True)
    g = bp.global_statistics(want_coef_cov=True, want_confidence_sigma=True)
    n, q = bp.n, bp.q
    assert (np.asarray(g["status"]) == np.asarray(st["status"])).all()
    ok = np.asarray(st["status"]) == 0
    assert ok.mean() >= 0.9
    # two factorisations of one matrix (QR of H vs QR of W Phi + Cholesky of the Schur complement) agree to rounding times
    # the conditioning: 1e-12 for the reference's models; the generic shape's Cov(alpha) spans six orders of magnitude
    # (measured 1.5e-12 on an MI355X)
    tol = 1e-11 if case == "generic" else 1e-12
    for b in np.nonzero(ok)[0]:
        cov = st["cov"][b]
        assert abs(g["reduced_chi2"][b] - st["reduced_chi2"][b]) <= 1e-12 * st["reduced_chi2"][b]
        assert _rel(g["cov_alpha"][b], cov[n:, n:]) <= tol, (name, b)
        assert _rel(g["coef_cov"][b, 0], cov[:n, :n]) <= tol, (name, b)
        assert _rel(g["coef_alpha_cov"][b, 0], cov[:n, n:]) <= tol, (name, b)
        assert _rel(g["conf_sigma"][b, 0], st["conf_sigma"][b]) <= tol, (name, b)
    assert g["dof"] == st["dof"]
    bp.close()


# ---- 2. small global fits: the device against the oracle's FitStatistics of the stacked problem ----
@pytest.mark.parametrize("shape", ["S2_n3_q2", "S4_n2_q2"])
@pytest.mark.parametrize("weighted", [False, True])
def test_small_global_fits_match_the_oracle_stacked_statistics(shape, weighted):
    rng = np.random.default_rng(17)
    m = 120
    x = np.linspace(0.0, 10.0, m)
    if shape == "S2_n3_q2":
        S, alpha = 2, np.array([0.8, 3.5])
        mdl = double_exp_builder_model(x, alpha)
    else:
        S, alpha = 4, np.array([0.9, 4.0])
        mdl = two_exp_model(x, alpha)
    Y = global_data(rng, mdl, x, alpha, S, 0.05)
    w = (0.5 + rng.random(m)) if weighted else None
    bp = vp.BatchProblem(mdl, Y[None], x=x, weights=w)
    a_fit, C_fit, rep = bp.fit((alpha * 1.1)[None])
    assert rep["termination"][0] > 0
    g = bp.global_statistics(want_coef_cov=True, want_confidence_sigma=True)
    _Phi, _dPhi, pb, pp = desc_columns(mdl, x, a_fit[0])
    d = dict(n=bp.n, q=bp.q, pb=pb, pp=pp, ev=lambda t, a: O.eval_phi(mdl, t, a),
             dv=lambda t, a: desc_columns(mdl, t, a)[1], a=a_fit[0], t=x, Y=Y, w=w, C=C_fit[0])
    C_or, st = oracle_stacked_stats(d)
    assert _rel(C_fit[0], C_or) <= 1e-10
    caa, ccs, cca = split(st["cov"], bp.n, S)
    assert int(g["status"][0]) == 0 and g["dof"] == st["dof"]
    assert abs(g["reduced_chi2"][0] - st["reduced_chi2"]) <= 1e-9 * st["reduced_chi2"]
    assert _rel(g["cov_alpha"][0], caa) <= 1e-9
    assert _rel(g["coef_cov"][0], ccs) <= 1e-9
    assert _rel(g["coef_alpha_cov"][0], cca) <= 1e-9
    assert _rel(g["conf_sigma"][0], st["conf_sigma"].reshape(S, m)) <= 1e-9
    # the solver surface
    b = vp.SeparableProblemBuilder.mrhs(mdl).observations(np.ascontiguousarray(Y.T))
    prob = (b.weights(w) if weighted else b).build()
    prob.set_params(alpha * 1.1)
    res, gs = vp.LevMarSolver.default().fit_with_global_statistics(prob)
    assert res.was_successful()
    assert _rel(gs.nonlinear_parameters_covariance_matrix(), caa) <= 1e-7
    assert gs.linear_coefficients_variance().shape == (bp.n, S)
    assert _rel(gs.linear_coefficients_variance(), np.diagonal(ccs, axis1=1, axis2=2).T) <= 1e-7
    assert np.allclose(np.diag(gs.nonlinear_parameters_correlation_matrix()), 1.0)
    assert abs(gs.regression_standard_error() ** 2 - gs.reduced_chi2()) <= 1e-14 * gs.reduced_chi2()
    from scipy import stats as _st
    rad = gs.confidence_band_radius(0.9)
    assert rad.shape == (m, S)
    assert _rel(rad, _st.t.ppf(0.95, st["dof"]) * st["conf_sigma"].reshape(S, m).T) <= 1e-7
    with pytest.raises(ValueError):
        vp.LevMarSolver.default().fit_with_statistics(prob)
    bp.close()


# ---- 3. larger S on the specialised MRHS kernel sets, against the block formulas at the device's alpha and C ----
@pytest.mark.parametrize("cfg", ["S64_m1024", "configs2"])
def test_large_global_fits_match_the_block_formulas(cfg):
    rng = np.random.default_rng(23)
    if cfg == "configs2":
        d = synth.mrhs_triple_exp(S=16384, m=2048)
        x, Y, guess = d["x"], d["Y"] + 0.5 * rng.standard_normal(d["Y"].shape), d["tau_guess"]
        mdl = vp.multi_exponential_model(x, guess)
        w, band_rhs = None, np.arange(0, 16384, 127)
    else:
        x = np.linspace(0.0, 12.0, 1024)
        mdl = double_exp_builder_model(x, [1.0, 4.0])
        Y = global_data(rng, mdl, x, np.array([1.0, 4.0]), 64, 0.02)
        guess, w, band_rhs = np.array([1.2, 3.5]), np.linspace(0.5, 2.0, 1024), None
    bp = vp.BatchProblem(mdl, Y[None], x=x, weights=w)
    a_fit, C_fit, rep = bp.fit(guess[None])
    assert rep["termination"][0] > 0
    g = bp.global_statistics(want_coef_cov=True, want_confidence_sigma=True)
    Phi, dPhi, pb, pp = desc_columns(mdl, x, a_fit[0])
    check_against_blocks(g, 0, Phi, dPhi, pb, pp, bp.q, w, C_fit[0], Y, 1e-9, band_rhs=band_rhs)
    bp.close()


# ---- 4. every route ----
def test_generic_descriptor_shape_with_three_rhs():
    rng = np.random.default_rng(8)
    x = 8.0 * np.arange(600) / 599 + 0.05
    mdl, alpha = generic_model(x)
    Y = global_data(rng, mdl, x, alpha, 3, 1e-2)
    w = np.linspace(0.5, 2.0, 600)
    bp = vp.BatchProblem(mdl, Y[None], x=x, weights=w)
    a_fit, C_fit, rep = bp.fit((alpha * 1.02)[None])
    assert rep["termination"][0] > 0
    g = bp.global_statistics(want_coef_cov=True, want_confidence_sigma=True)
    Phi, dPhi, pb, pp = desc_columns(mdl, x, a_fit[0])
    check_against_blocks(g, 0, Phi, dPhi, pb, pp, 4, w, C_fit[0], Y, 1e-9)
    bp.close()


def test_external_handle_fitted_by_fit_with_model():
    rng = np.random.default_rng(9)
    n, q, pb, pp, ev, dv, a_true = MODELS["damped_cos"]()
    S, B, m = 3, 2, 200
    t = np.linspace(0.0, 6.0, m)
    Ys = np.stack([(rng.uniform(0.5, 2.0, (S, n)) @ ev(t, a_true)) + 0.02 * rng.standard_normal((S, m)) for _ in range(B)])
    w = 0.5 + rng.random(m)
    bp = vp.BatchProblem(vp.ExternalModel(n, q, list(zip(pb, pp))), Ys, weights=w)

    def evaluate(alpha, _want):
        return (np.stack([ev(t, a) for a in alpha]), np.stack([dv(t, a) for a in alpha]))

    a_fit, C_fit, rep, _steps = bp.fit_with_model(evaluate, np.tile(a_true * 1.05, (B, 1)))
    assert (rep["termination"] > 0).all()
    with pytest.raises(vp.VarproHipError) as e:  # the columns of the fitted point are not known yet
        bp.global_statistics()
    assert e.value.code == _lib.VP_ERR_INVALID
    Phi, dPhi = evaluate(a_fit, None)
    bp.set_params_with_basis(a_fit, Phi, dPhi)
    g = bp.global_statistics(want_coef_cov=True, want_confidence_sigma=True)
    C_now = bp.linear_coefficients()
    for b in range(B):
        check_against_blocks(g, b, Phi[b], dPhi[b], pb, pp, q, w, C_now[b], Ys[b], 1e-9)
    bp.close()


def test_fp32_handle():
    rng = np.random.default_rng(10)
    x = np.linspace(0.0, 12.0, 1024)
    alpha = np.array([1.0, 4.0])
    mdl64 = double_exp_builder_model(x, alpha)
    Y = global_data(rng, mdl64, x, alpha, 3, 0.05)
    mdl = SeparableModel(["tau1", "tau2"], [basis.EXP_DECAY, basis.EXP_DECAY, basis.CONST], [(0,), (1,), ()],
                         x.astype(np.float32), alpha.astype(np.float32), dtype=np.float32)
    bp = vp.BatchProblem(mdl, Y[None].astype(np.float32), x=x.astype(np.float32))
    a_fit, C_fit, rep = bp.fit((alpha * 1.1)[None].astype(np.float32))
    g = bp.global_statistics(want_coef_cov=True, want_confidence_sigma=True)
    assert g["cov_alpha"].dtype == np.float32 and g["conf_sigma"].dtype == np.float32
    a64 = a_fit[0].astype(np.float64)
    Phi, dPhi, pb, pp = desc_columns(mdl64, x, a64)
    C64 = C_fit[0].astype(np.float64)
    check_against_blocks(g, 0, Phi, dPhi, pb, pp, 2, None, C64, Y.astype(np.float32).astype(np.float64), 1e-4)
    bp.close()


def test_torch_tensors_null_outputs_and_repeatability():
    import torch
    rng = np.random.default_rng(12)
    x = np.linspace(0.0, 12.0, 1024)
    alpha = np.array([1.0, 4.0])
    mdl = double_exp_builder_model(x, alpha)
    Y = np.stack([global_data(rng, mdl, x, alpha, 5, 0.02) for _ in range(3)])
    w = np.linspace(0.5, 2.0, 1024)
    a = np.array([[1.01, 3.9], [0.99, 4.1], [1.0, 4.0]])
    bp = vp.BatchProblem(mdl, Y, x=x, weights=w)
    bp.set_params(a)
    g1 = bp.global_statistics(want_coef_cov=True, want_confidence_sigma=True)
    g2 = bp.global_statistics(want_coef_cov=True, want_confidence_sigma=True)
    g0 = bp.global_statistics(want_coef_cov=False, want_confidence_sigma=False)
    for k in ("cov_alpha", "reduced_chi2", "coef_cov", "coef_alpha_cov", "conf_sigma", "status"):
        assert np.array_equal(g1[k], g2[k]), k
    for k in ("cov_alpha", "reduced_chi2", "status"):
        assert np.array_equal(g0[k], g1[k]), k
    assert g0["coef_cov"] is None and g0["coef_alpha_cov"] is None and g0["conf_sigma"] is None
    dev = torch.device("cuda:0")
    bt = vp.BatchProblem(mdl, torch.as_tensor(Y, device=dev), x=torch.as_tensor(x, device=dev),
                         weights=torch.as_tensor(w, device=dev))
    bt.set_params(torch.as_tensor(a, device=dev))
    gt = bt.global_statistics(want_coef_cov=True, want_confidence_sigma=True)
    torch.cuda.synchronize()
    for k in ("cov_alpha", "reduced_chi2", "coef_cov", "coef_alpha_cov", "conf_sigma", "status"):
        assert np.array_equal(gt[k].cpu().numpy(), g1[k]), k
    bt.close()
    bp.close()


# ---- 5. status 4 and refusals ----
def test_status_4_and_refusals():
    # a rank-deficient Phi: a zero basis column
    rng = np.random.default_rng(13)
    m, S = 50, 2
    t = np.linspace(0.0, 5.0, m)
    Phi = np.stack([np.exp(-t / 1.5), np.zeros(m), np.ones(m)])[None]
    dPhi = np.stack([t / 1.5 ** 2 * np.exp(-t / 1.5)])[None]
    Y = rng.standard_normal((1, S, m))
    bp = vp.BatchProblem(vp.ExternalModel(3, 1, [(0, 0)]), Y)
    bp.set_params_with_basis(np.array([[1.5]]), Phi, dPhi)
    g = bp.global_statistics(want_coef_cov=True, want_confidence_sigma=True)
    assert int(g["status"][0]) == 4
    assert np.isnan(g["cov_alpha"]).all() and np.isnan(g["reduced_chi2"]).all() and np.isnan(g["conf_sigma"]).all()
    bp.close()
    # m S <= n S + q
    xs = np.linspace(0, 1, 4)
    mdl = double_exp_builder_model(xs, [0.3, 2.0])
    bp = vp.BatchProblem(mdl, rng.standard_normal((1, 2, 4)), x=xs)
    with pytest.raises(vp.VarproHipError) as e:  # no parameters yet
        bp.global_statistics()
    assert e.value.code == _lib.VP_ERR_INVALID
    bp.set_params(np.array([[0.3, 2.0]]))
    g = bp.global_statistics()
    assert int(g["status"][0]) == 4 and g["dof"] == 0
    bp.close()
    # right-hand sides sharded over ranks
    x = np.linspace(0.0, 12.0, 1024)
    mdl = double_exp_builder_model(x, [1.0, 4.0])
    bp = vp.BatchProblem(mdl, global_data(rng, mdl, x, np.array([1.0, 4.0]), 4, 0.02)[None], x=x)
    bp.set_params(np.array([[1.0, 4.0]]))
    cb = _lib.ALLREDUCE_FN(lambda ptr, count, stream, user: 0)
    _lib.check(bp.lib.vp_set_rhs_allreduce(bp._h, cb, None, ctypes.c_int64(8)))
    with pytest.raises(vp.VarproHipError) as e:
        bp.global_statistics()
    assert e.value.code == _lib.VP_ERR_UNSUPPORTED
    _lib.check(bp.lib.vp_set_rhs_allreduce(bp._h, _lib.ALLREDUCE_FN(0), None, 0))
    assert int(bp.global_statistics()["status"][0]) == 0
    bp.close()


# ---- 6. calibration: predicted spread of the fitted alpha against the empirical spread over replicas ----
def test_calibration_over_512_replicas():
    rng = np.random.default_rng(2024)
    B, S, m, sigma = 512, 8, 256, 0.01
    x = np.linspace(0.0, 10.0, m)
    alpha = np.array([1.0, 4.0])
    mdl = double_exp_builder_model(x, alpha)
    Phi = O.eval_phi(mdl, x, alpha)
    Ct = rng.uniform(0.5, 1.5, (S, 3))
    Y = (Ct @ Phi)[None] + sigma * rng.standard_normal((B, S, m))
    bp = vp.BatchProblem(mdl, Y, x=x)
    a_fit, _C, rep = bp.fit(np.tile(alpha * 1.05, (B, 1)))
    assert (rep["termination"] > 0).all()
    g = bp.global_statistics(want_coef_cov=False)
    assert (np.asarray(g["status"]) == 0).all()
    pred = np.sqrt(np.diagonal(g["cov_alpha"], axis1=1, axis2=2)).mean(0)
    emp = a_fit.std(0, ddof=1)
    assert (np.abs(emp / pred - 1.0) <= 0.10).all(), (emp, pred)
    assert abs(np.mean(g["reduced_chi2"]) / sigma ** 2 - 1.0) <= 0.05
    bp.close()
