"""CPU tier: the block formulas of the global-fit statistics (vp_global_statistics) pinned against
(a) a dense numpy restatement of FitStatistics::try_calculate on the stacked single-RHS problem (np.linalg.qr of the whole
(m S) x (n S + q) matrix H) and (b) the CPU oracle's own FitStatistics on that stacked problem, built through its
external-model hook.  The GPU tier (test_gpu_global_statistics.py) checks the device against the same functions."""
import numpy as np
import pytest

from oracle import oracle as O


def block_stats(Phi, dPhi, pb, pp, q, w, C, Y, band_rhs=None):
    """The block formulas.  Phi (n, m) and dPhi (P, m) UNweighted; pair p = (basis pb[p], parameter pp[p]); w (m,) or None;
    C (S, n); Y (S, m).  -> dict(cov_alpha, chi2, coef_cov (S,n,n), coef_alpha_cov (S,n,q), band, dof); band (S, m), or
    only the rows of the right-hand sides band_rhs"""
    n, m = Phi.shape
    S = C.shape[0]
    P = len(pb)
    W = np.ones(m) if w is None else np.asarray(w, dtype=np.float64)
    Qf, R = np.linalg.qr((Phi * W).T)                      # W Phi = Q R
    Ri = np.linalg.inv(R)
    WD = dPhi * W                                          # (P, m)
    E = Ri @ (Qf.T @ WD.T)                                 # (n, P)
    G = WD.T - Qf @ (Qf.T @ WD.T)                          # (m, P): P_perp W dPhi_p
    F = dPhi.T - Phi.T @ E                                 # (m, P) unweighted
    A = C.T @ C                                            # sum_s c_s c_s^T
    M = np.zeros((q, q))
    GG = G.T @ G
    for p in range(P):
        for r in range(P):
            M[pp[p], pp[r]] += GG[p, r] * A[pb[p], pb[r]]
    res = (Y - C @ Phi) * W
    dof = m * S - n * S - q
    chi2 = (res ** 2).sum() / dof
    cov_a = chi2 * np.linalg.inv(M)
    K = np.zeros((S, n, q))
    Cb = C if band_rhs is None else C[band_rhs]
    U = np.zeros((Cb.shape[0], m, q))
    for p in range(P):
        K[:, :, pp[p]] += C[:, pb[p], None] * E[None, :, p]
        U[:, :, pp[p]] += Cb[:, pb[p], None] * F[None, :, p]
    RR = Ri @ Ri.T
    coef_cov = chi2 * RR[None] + np.einsum("sak,kl,sbl->sab", K, cov_a, K)
    coef_alpha = -np.einsum("sak,kl->sal", K, cov_a)
    lev = ((Ri.T @ Phi) ** 2).sum(0)                       # ||R^-T phi_i^T||^2
    band = np.sqrt(chi2 * lev[None] + np.einsum("sik,kl,sil->si", U, cov_a, U))
    return dict(cov_alpha=cov_a, chi2=chi2, coef_cov=coef_cov, coef_alpha_cov=coef_alpha, band=band, dof=dof)


def stacked(Phi, dPhi, pb, pp, q, w, C):
    """the equivalent single-RHS problem: Phi_st (n S, m S) [j][i], dPhi_st(k) (n S, m S), weights (m S,)"""
    n, m = Phi.shape
    S = C.shape[0]
    Phi_st = np.zeros((n * S, m * S))
    for s in range(S):
        Phi_st[s * n:(s + 1) * n, s * m:(s + 1) * m] = Phi

    def dk(k):
        D = np.zeros((n * S, m * S))
        for p in range(len(pb)):
            if pp[p] == k:
                for s in range(S):
                    D[s * n + pb[p], s * m:(s + 1) * m] += dPhi[p]
        return D

    W = np.tile(np.ones(m) if w is None else w, S)
    return Phi_st, dk, W


def dense_stats(Phi, dPhi, pb, pp, q, w, C, Y):
    """FitStatistics::try_calculate (src/statistics/mod.rs:352-441) on the stacked problem, dense"""
    n, m = Phi.shape
    S = C.shape[0]
    Phi_st, dk, W = stacked(Phi, dPhi, pb, pp, q, w, C)
    c = C.reshape(-1)
    J = np.concatenate([Phi_st.T, np.stack([dk(k).T @ c for k in range(q)], 1)], 1)  # (mS, nS + q) unweighted
    H = J * W[:, None]
    _, R = np.linalg.qr(H)
    Ri = np.linalg.inv(R)
    r = (Y.reshape(-1) - Phi_st.T @ c) * W
    dof = m * S - n * S - q
    chi2 = r @ r / dof
    cov = chi2 * Ri @ Ri.T
    band = np.sqrt(np.einsum("ia,ab,ib->i", J, cov, J)).reshape(S, m)
    return cov, chi2, band


def split(cov, n, S):
    ns = n * S
    return (cov[ns:, ns:], np.stack([cov[s * n:(s + 1) * n, s * n:(s + 1) * n] for s in range(S)]),
            np.stack([cov[s * n:(s + 1) * n, ns:] for s in range(S)]))


# ---- small models with explicit derivatives: (n, q, pairs, eval(t, a) -> Phi (n, m), derivs(t, a) -> dPhi (P, m)) ----
def model_two_exp_offset():  # separate parameters, a constant basis
    pb, pp = [0, 1], [0, 1]

    def ev(t, a):
        return np.stack([np.exp(-t / a[0]), np.exp(-t / a[1]), np.ones_like(t)])

    def dv(t, a):
        return np.stack([t / a[0] ** 2 * np.exp(-t / a[0]), t / a[1] ** 2 * np.exp(-t / a[1])])

    return 3, 2, pb, pp, ev, dv, np.array([0.7, 2.5])


def model_damped_cos():  # a parameter shared by two bases, a basis that depends on two parameters
    pb, pp = [0, 0, 1, 1], [0, 1, 0, 1]

    def ev(t, a):
        e = np.exp(-a[0] * t)
        return np.stack([e * np.cos(a[1] * t), e * np.sin(a[1] * t), np.ones_like(t)])

    def dv(t, a):
        e = np.exp(-a[0] * t)
        c, s = np.cos(a[1] * t), np.sin(a[1] * t)
        return np.stack([-t * e * c, -t * e * s, -t * e * s, t * e * c])

    return 3, 2, pb, pp, ev, dv, np.array([0.4, 2.0])


def model_shared_two():  # n = 2: exp(-a0 t), exp(-(a0 + a1) t)
    pb, pp = [0, 1, 1], [0, 0, 1]

    def ev(t, a):
        return np.stack([np.exp(-a[0] * t), np.exp(-(a[0] + a[1]) * t)])

    def dv(t, a):
        e0, e1 = np.exp(-a[0] * t), np.exp(-(a[0] + a[1]) * t)
        return np.stack([-t * e0, -t * e1, -t * e1])

    return 2, 2, pb, pp, ev, dv, np.array([0.5, 1.2])


MODELS = {"two_exp_offset": model_two_exp_offset, "damped_cos": model_damped_cos, "shared_two": model_shared_two}


def make_data(rng, model, S, m, weighted, noise=0.02):
    n, q, pb, pp, ev, dv, a = model()
    t = np.linspace(0.0, 6.0, m)
    Phi, dPhi = ev(t, a), dv(t, a)
    Ctrue = rng.uniform(0.5, 2.0, (S, n))
    Y = Ctrue @ Phi + noise * rng.standard_normal((S, m))
    w = (0.5 + rng.random(m)) if weighted else None
    W = np.ones(m) if w is None else w
    C = np.linalg.lstsq((Phi * W).T, (Y * W).T, rcond=None)[0].T  # the fitted coefficients at this alpha
    return dict(n=n, q=q, pb=pb, pp=pp, ev=ev, dv=dv, a=a, t=t, Phi=Phi, dPhi=dPhi, Y=Y, w=w, C=C)


def _rel(x, ref):
    return np.abs(np.asarray(x) - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("S,weighted", [(1, False), (3, True), (7, True)])
def test_block_formulas_equal_the_dense_stacked_problem(name, S, weighted):
    rng = np.random.default_rng(11 + S)
    d = make_data(rng, MODELS[name], S, 60, weighted)
    blk = block_stats(d["Phi"], d["dPhi"], d["pb"], d["pp"], d["q"], d["w"], d["C"], d["Y"])
    cov, chi2, band = dense_stats(d["Phi"], d["dPhi"], d["pb"], d["pp"], d["q"], d["w"], d["C"], d["Y"])
    caa, ccs, cca = split(cov, d["n"], S)
    assert abs(blk["chi2"] - chi2) <= 1e-13 * chi2
    assert _rel(blk["cov_alpha"], caa) <= 1e-9
    assert _rel(blk["coef_cov"], ccs) <= 1e-9
    assert _rel(blk["coef_alpha_cov"], cca) <= 1e-9
    assert _rel(blk["band"], band) <= 1e-9


def oracle_stacked_stats(d):
    """the oracle's FitStatistics of the stacked problem (external-model hook), at alpha = d['a']"""
    n, q, S, m = d["n"], d["q"], d["C"].shape[0], d["t"].size
    t = d["t"]

    def ev(a):
        return stacked(d["ev"](t, a), d["dv"](t, a), d["pb"], d["pp"], q, d["w"], d["C"])[0]

    def dk(a, k):
        return stacked(d["ev"](t, a), d["dv"](t, a), d["pb"], d["pp"], q, d["w"], d["C"])[1](k)

    w_st = None if d["w"] is None else np.tile(d["w"], S)
    prob = O.Problem(O.make_shape_desc(n * S, q), None, d["Y"].reshape(-1), w=w_st, external=(ev, dk))
    prob.set_params(d["a"])
    st = prob.statistics()
    assert st is not None
    return prob.linear_coefficients().reshape(S, n), st


@pytest.mark.parametrize("name,S", [("two_exp_offset", 2), ("damped_cos", 2), ("shared_two", 4)])
@pytest.mark.parametrize("weighted", [False, True])
def test_block_formulas_equal_the_oracle_fit_statistics_of_the_stacked_problem(name, S, weighted):
    rng = np.random.default_rng(5)
    d = make_data(rng, MODELS[name], S, 40, weighted)
    C_or, st = oracle_stacked_stats(d)
    assert _rel(C_or, d["C"]) <= 1e-10  # the oracle's stacked solve finds the same coefficients
    blk = block_stats(d["Phi"], d["dPhi"], d["pb"], d["pp"], d["q"], d["w"], C_or, d["Y"])
    caa, ccs, cca = split(st["cov"], d["n"], S)
    assert st["dof"] == blk["dof"]
    assert abs(blk["chi2"] - st["reduced_chi2"]) <= 1e-12 * st["reduced_chi2"]
    assert _rel(blk["cov_alpha"], caa) <= 1e-8
    assert _rel(blk["coef_cov"], ccs) <= 1e-8
    assert _rel(blk["coef_alpha_cov"], cca) <= 1e-8
    assert _rel(blk["band"], st["conf_sigma"].reshape(S, -1)) <= 1e-8
