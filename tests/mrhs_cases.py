"""Cases and references of the per-kernel-set tests of the global-fit path, several right-hand sides sharing one parameter
vector (vp_mrhs.hpp: the factor kernel, the streaming kernel, the two workgroup-cooperative kernels, the LM step kernel;
tests/test_mrhs_cases_host.py, tests/test_gpu_global_fit_sets.py).

The set records, model shapes, the case record, the seeds and the way the data are made are those of tests/stats_cases.py,
extended by a number S of right-hand sides: per problem, Y has S columns made from the shape's truth with random
coefficients.  The `_wide` shapes and the noise exception of five exponentials are those of tests/fit_cases.py.  Every case
names its set (vp_debug_kernel_set) and the record of vp_debug_last_global it expects after each call,
(factor_waves, step_waves, fit_stream, eval_stream, gx_fit, gx_eval, 0, 0), computed from the launchers' rules, which are
restated ONCE below.  Per registered set with multiple-right-hand-side kernels, of capacity 64 R:

  A  m = 64 R      uniform grid   no weights  B 5, S 3     2-element loads, exponential recurrence, one workgroup per problem
                                                           with idle column waves; four-wave factor / step where R % 8 == 0;
                                                           fp64 R = 32: the cooperative DMA kernel in the fit, the cooperative
                                                           output kernel with and without J
  B  m = 64 R - 1  jittered grid  shared w    B 5, S 9     element-wise loads, no recurrence, weights; two streaming workgroups,
                                                           the second holding one column; fp64 R = 32: the fall-back from the
                                                           cooperative kernels to the streaming kernel
  C  the set's     uniform grid   no weights  B 1025, S 2  the one-wave factor and step kernels: only where R % 8 == 0 and the
     smallest even m                                       one-wave form exists.  Five distinct problems repeated round-robin
                                                           (b % 5), each with its own parameters; all 1025 results are compared
  P  per-problem grids and weights, B 5, S 3: one small and one R = 16 set of each family and dtype

References are computed once per case (functools.lru_cache) and returned read-only."""
import collections
import ctypes as C
import functools

import numpy as np

import fit_cases as FC
from oracle import oracle as O
from stats_cases import EPS32, F32, F64, FP32_UNIT_MARGIN, NP_DTYPE, SHAPES, _seed, case, case_id, make_model, me_set, rt_set
from varpro_amd._lib import FAMILY_MULTIEXP

NB = 5  # distinct problems of a case
STREAM, COOP_DMA, COOP_OUT_J, COOP_OUT, GENERIC = 1, 2, 3, 4, 5  # vp_debug_last_global: stream codes
# cls, the stats_cases record, right-hand sides, problems of the handle (problem b of the handle is distinct problem b % NB)
GCase = collections.namedtuple("GCase", "cls case S B")


def gcase_id(gc):
    return "%s-S%d-B%d-%s" % (gc.cls, gc.S, gc.B, case_id(gc.case))


# ---- the launchers' rules (vp_mrhs.hpp), restated once ---------------------------------------------------------------------
def set_columns(rec):
    """(N basis functions, P derivative pairs, bytes per element) of a set's model"""
    dtype, fam, a, b, c, _R, _W, _gen = rec
    n, p = (a + b, a) if fam == FAMILY_MULTIEXP else (a, c)
    return n, p, 8 if dtype == F64 else 4


def one_wave_spills(rec):
    """mrhs_one_wave_spills: the N + 1 + P columns of R rows per lane do not fit the 512 VGPRs of one wave"""
    n, p, size = set_columns(rec)
    return (n + 1 + p) * rec[5] * (size // 4) > 400


def has_one_wave_form(rec):
    """launch_mrhs_factor / launch_mrhs_lm can take the one-wave kernels at all AND have a four-wave form to choose from
    (the sets of class C)"""
    return rec[5] % 8 == 0 and not one_wave_spills(rec)


def waves(rec, B):
    """waves per problem of mrhs_factor_kernel and mrhs_step_kernel: four where R % 8 == 0 and (B <= 1024 or the one-wave form
    spills), else one"""
    return 4 if rec[5] % 8 == 0 and (B <= 1024 or one_wave_spills(rec)) else 1


def mrhs_gx(S, cap=256):
    """workgroups per problem of a streaming pass: one per 8 columns, at most cap"""
    return max(1, min((S + 7) // 8, cap))


def gx_cap(rec):
    """mrhs_gx_cap: the cooperative DMA kernel of the fp64 R = 32 sets runs two workgroups per CU"""
    return 512 if is_coop(rec) else 256


def is_coop(rec):
    return rec[0] == F64 and rec[5] == 32


def eval_stream(rec, m, S, r_out=True, J_out=True):
    """(code, gx) of launch_mrhs_stream's MODE 1 pass: the cooperative output kernel on the fp64 R = 32 sets where `vec` holds
    (m even; the handle's own arrays are 16-byte aligned) and r or J is asked for, else the streaming kernel"""
    if is_coop(rec) and m % 2 == 0 and (r_out or J_out):
        return (COOP_OUT_J if J_out else COOP_OUT), mrhs_gx(S, 512)
    return STREAM, mrhs_gx(S)


def fit_stream(rec, m, S):
    """(code, gx) of the MODE 0 pass of the fit"""
    return (COOP_DMA if is_coop(rec) and m % 2 == 0 else STREAM), mrhs_gx(S, gx_cap(rec))


def record(gc, evaluated=None, fitted=False):
    """the record of vp_debug_last_global of a fresh handle of the case after an optional evaluation -- evaluated = (r_out,
    J_out), the outputs asked for -- and an optional fit, in that order.  (The fit factors inside the step kernel: the factor
    launcher runs in evaluations only.)"""
    rec, m = gc.case.set, gc.case.m
    out = [0] * 8
    if evaluated is not None:
        out[0] = waves(rec, gc.B)
        out[3], out[5] = eval_stream(rec, m, gc.S, *evaluated)
    if fitted:
        out[1] = waves(rec, gc.B)
        out[2], out[4] = fit_stream(rec, m, gc.S)
    return tuple(out)


# ---- the sets with multiple-right-hand-side kernels: shape, dtype, record maker, rows per lane ------------------------------
def _me(nexp, off, dtype=F64):
    return lambda R: me_set(dtype, nexp, off, R)


def _rt(n, q, p):
    return lambda R: rt_set(n, q, p, R)


GLOBAL_SETS = [
    ("me2o", F64, _me(2, 1), [2, 4, 8, 12, 16, 20, 32]),
    ("me1o", F64, _me(1, 1), [2, 8, 16, 24, 32]),
    ("me1", F64, _me(1, 0), [2, 16]),
    ("me2", F64, _me(2, 0), [2, 16]),
    ("me3o_wide", F64, _me(3, 1), [2, 8, 16, 20, 32]),
    ("me3", F64, _me(3, 0), [2]),
    ("me2o", F32, _me(2, 1, F32), [2, 8, 16, 32]),
    ("me5o_wide", F32, _me(5, 1, F32), [2]),
    ("rate1", F64, _rt(1, 1, 1), [2, 16]),
    ("rate1o", F64, _rt(2, 1, 1), [2, 16]),
    ("rate2", F64, _rt(2, 2, 2), [2, 16]),
    ("cos1", F64, _rt(1, 2, 2), [2, 16]),
    ("cos2", F64, _rt(2, 4, 4), [2, 16]),
    ("rate3", F64, _rt(3, 3, 3), [2, 16]),
    ("rate3o", F64, _rt(4, 3, 3), [2]),
    ("cos_rate2", F64, _rt(3, 4, 4), [2]),
    ("cos_rate2o", F64, _rt(4, 4, 4), [2]),
    ("dexp_unit", F64, _rt(3, 2, 2), [2, 4, 8, 12, 16]),
    ("oleary", F64, _rt(2, 3, 4), [2, 4, 8, 12, 16]),
]


def _cases():
    out = []
    for shape, dtype, mk, sizes in GLOBAL_SETS:
        below = 0  # capacity of the next smaller set of the key
        for R in sizes:
            cap, rec = 64 * R, mk(R)
            out.append(GCase("A", FC._case(shape, dtype, cap, rec), 3, NB))
            out.append(GCase("B", FC._case(shape, dtype, cap - 1, rec, weights="shared", uniform=False), 9, NB))
            if has_one_wave_form(rec):
                out.append(GCase("C", FC._case(shape, dtype, below + 2 if below else FC.SMALL_M[shape], rec), 2, 1025))
            below = cap
    return out


SET_CASES = _cases()
PER_PROBLEM_CASES = [GCase("P", case(shape, dtype, m, rec, weights="per", grid="per"), 3, NB) for shape, dtype, m, rec in [
    ("me2o", F64, 127, me_set(F64, 2, 1, 2)), ("me2o", F64, 900, me_set(F64, 2, 1, 16)),
    ("me2o", F32, 100, me_set(F32, 2, 1, 2)), ("me2o", F32, 900, me_set(F32, 2, 1, 16)),
    ("dexp_unit", F64, 100, rt_set(3, 2, 2, 2)), ("oleary", F64, 900, rt_set(2, 3, 4, 16))]]
CASES = SET_CASES + PER_PROBLEM_CASES
IDS = [gcase_id(gc) for gc in CASES]


# ---- data ------------------------------------------------------------------------------------------------------------------
def _ro(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case_data(gc):
    """the NB distinct problems of a case in the handle's dtype: x (m,) or (NB, m), Y (NB, S, m), w None / (m,) / (NB, m),
    alpha (NB, q) = the truth times 1.00 .. 1.04 (the evaluation point), guess (NB, q) = the truth times 0.95 .. 1.05 (the
    start of the fit); every column has its own coefficients and noise.  Grids and weights as stats_cases.case_data"""
    c = gc.case
    s, T = SHAPES[c.shape], NP_DTYPE[c.dtype]
    rng = np.random.default_rng([_seed(c), gc.S])
    n, q = len(s.kinds), len(s.truth)
    x = np.linspace(0.0, s.span, c.m)
    if not c.uniform and c.grid != "per":  # every interior point moved by up to 0.4 of the spacing: still increasing
        x[1:-1] += 0.8 * (rng.random(c.m - 2) - 0.5) * s.span / (c.m - 1)
    if c.grid == "per":  # every problem its own span, every grid non-uniform
        x = np.stack([np.sort(rng.random(c.m)) * s.span * (1.0 + 0.05 * b) for b in range(NB)])
    x = np.ascontiguousarray(x, dtype=T)
    mdl = make_model(c.shape, x if x.ndim == 1 else x[0], T)
    coef = rng.uniform(5.0, 50.0, (NB, gc.S, n))
    Y = np.stack([coef[b] @ O.eval_phi(mdl, x if x.ndim == 1 else x[b], s.truth) for b in range(NB)])
    Y = Y + c.noise * np.abs(Y).max((1, 2), keepdims=True) * rng.standard_normal(Y.shape)
    alpha = np.asarray(s.truth) * rng.uniform(1.0, 1.04, (NB, q))
    guess = np.asarray(s.truth) * rng.uniform(0.95, 1.05, (NB, q))
    w = {None: None, "shared": rng.uniform(0.5, 1.5, c.m), "per": rng.uniform(0.5, 1.5, (NB, c.m))}[c.weights]
    cc = lambda a: _ro(np.ascontiguousarray(a, dtype=T))  # noqa: E731
    return dict(model=mdl, x=cc(x), Y=cc(Y), alpha=cc(alpha), guess=cc(guess), w=None if w is None else cc(w))


def handle_inputs(gc):
    """the arrays of the handle's gc.B problems: problem b is distinct problem b % NB -> dict(x, Y, w, alpha, guess, index)"""
    d = case_data(gc)
    idx = np.arange(gc.B) % NB
    per = lambda a: a if a is None or a.ndim == 1 else np.ascontiguousarray(a[idx])  # noqa: E731
    return dict(model=d["model"], x=per(d["x"]), w=per(d["w"]), Y=np.ascontiguousarray(d["Y"][idx]),
                alpha=np.ascontiguousarray(d["alpha"][idx]), guess=np.ascontiguousarray(d["guess"][idx]), index=idx)


def problem_inputs(d, b):
    """(x (m,), Y (S, m), w) of distinct problem b as fp64 copies of the handle's inputs"""
    x = d["x"] if d["x"].ndim == 1 else d["x"][b]
    w = None if d["w"] is None else (d["w"] if d["w"].ndim == 1 else d["w"][b])
    return x.astype(np.float64), d["Y"][b].astype(np.float64), None if w is None else w.astype(np.float64)


def weighted_data(d, b):
    _x, Y, w = problem_inputs(d, b)
    return Y if w is None else Y * w


def handle_grid_uniform(gc):
    d = case_data(gc)
    return all(FC.grid_is_uniform(g) for g in (d["x"] if d["x"].ndim == 2 else [d["x"]]))


# ---- references ------------------------------------------------------------------------------------------------------------
def _oracle_problem(gc, b, alpha):
    d = case_data(gc)
    x, Y, w = problem_inputs(d, b)
    p = O.Problem(d["model"], x, Y, w=w)
    p.set_params(np.asarray(alpha, dtype=np.float64))
    return p


@functools.lru_cache(maxsize=None)
def oracle_evaluate(gc):
    """the oracle at the case's alpha, distinct problem by distinct problem: dict(C (NB, S, n), r (NB, S m), J (NB, q, S m),
    cost (NB,), status (NB,)) -- r and J column-stacked as the reference's residual vector and Jacobian"""
    d = case_data(gc)
    out = dict(C=[], r=[], J=[], cost=[], status=[])
    for b in range(NB):
        p = _oracle_problem(gc, b, d["alpha"][b])
        r = p.residuals()
        out["status"].append(0 if r is not None else 1)
        out["C"].append(p.linear_coefficients())
        out["r"].append(r)
        out["J"].append(p.jacobian())
        out["cost"].append(0.5 * float(r @ r))
    return {k: _ro(np.array(v)) for k, v in out.items()}


def oracle_cost(gc, b, alpha):
    """the variable projection functional 1/2 |r_w(alpha)|^2 of distinct problem b over all columns, fp64 oracle"""
    r = _oracle_problem(gc, b, alpha).residuals()
    return np.inf if r is None else 0.5 * float(r @ r)


def scaled_cond_J(gc, b, alpha):
    """cond of the column-scaled (S m) x q Jacobian of distinct problem b at alpha: what the LM driver sees (scale_diag)"""
    J = _oracle_problem(gc, b, alpha).jacobian().T
    sv = np.linalg.svd(J / np.linalg.norm(J, axis=0), compute_uv=False)
    return float(sv[0] / sv[-1])


@functools.lru_cache(maxsize=None)
def oracle_fit(gc):
    """the oracle's own global fit of every distinct problem from the case's guess: dict(alpha (NB, q), C (NB, S, n),
    termination, n_evals, objective (NB,), trace: list of (rows, q + 4))"""
    d = case_data(gc)
    n = len(SHAPES[gc.case.shape].kinds)
    out = dict(alpha=[], C=[], termination=[], n_evals=[], objective=[], trace=[])
    for b in range(NB):
        p = _oracle_problem(gc, b, d["guess"][b])
        rep, tr = p.fit_trace(max_rows=16)
        out["alpha"].append(p.params())
        out["C"].append(p.linear_coefficients() if p.cached() else np.full((gc.S, n), np.nan))
        out["termination"].append(rep.termination)
        out["n_evals"].append(rep.n_evals)
        out["objective"].append(rep.objective)
        out["trace"].append(_ro(tr))
    return {k: (v if k == "trace" else _ro(np.array(v))) for k, v in out.items()}


def numpy_jacobian(model, x, Y, w, alpha):
    """the second witness of the oracle's Jacobian for several right-hand sides: J_k = -P_perp (W D_k c_s), column s after
    column s, with P_perp = I - Q Q^T from a QR of W Phi and c_s = lstsq(W Phi, w y_s) -> (q, S m)"""
    q = int(model.n_params)
    wv = np.ones(x.size) if w is None else w
    Pw = O.eval_phi(model, x, alpha).T * wv[:, None]
    Q = np.linalg.qr(Pw)[0]
    Cs = np.linalg.lstsq(Pw, (Y * wv).T, rcond=None)[0]  # (n, S)
    out = []
    for k in range(q):
        V = (O.eval_dphi(model, x, alpha, k).T * wv[:, None]) @ Cs  # (m, S)
        out.append(-(V - Q @ (Q.T @ V)).T.reshape(-1))
    return np.array(out)


EVAL_KEYS = FC.EVAL_KEYS


def eval_errors(got, ref, b, Yw):
    """the metric of the evaluation comparison for ONE problem -- got: C (S, n), r (S m), J (q, S m), cost of it; ref:
    oracle_evaluate's record, b the distinct problem -- the scales of fit_cases.eval_errors over all columns: C over max |C|, r
    over max |Y_w|, J_k over max |J_k| (the largest over k), cost over max(cost, 1e-6 |Y_w|^2)"""
    g = {k: np.asarray(got[k], dtype=np.float64) for k in EVAL_KEYS}
    q = ref["J"].shape[1]
    eJ = max(float(np.abs(g["J"][k].reshape(-1) - ref["J"][b, k]).max() / np.abs(ref["J"][b, k]).max()) for k in range(q))
    return dict(C=float(np.abs(g["C"] - ref["C"][b]).max() / np.abs(ref["C"][b]).max()),
                r=float(np.abs(g["r"].reshape(-1) - ref["r"][b]).max() / np.abs(Yw).max()), J=eJ,
                cost=float(abs(g["cost"] - ref["cost"][b]) / max(ref["cost"][b], 1e-6 * float((Yw ** 2).sum()))))


@functools.lru_cache(maxsize=None)
def numpy_evaluate_errors(gc, dtype):
    """per distinct problem: the errors of fit_cases.numpy_evaluate, run in `dtype` column by column (the cost summed in
    `dtype`), against the oracle, and cond(W Phi)"""
    d, ref = case_data(gc), oracle_evaluate(gc)
    T = np.dtype(dtype).type
    out = []
    for b in range(NB):
        x, Y, w = problem_inputs(d, b)
        ev = [FC.numpy_evaluate(d["model"], x, Y[s], w, d["alpha"][b].astype(np.float64), dtype) for s in range(gc.S)]
        cost = T(0)
        for e in ev:
            cost = T(cost + e["cost"])
        got = dict(C=np.stack([e["C"] for e in ev]), r=np.concatenate([e["r"] for e in ev]),
                   J=np.concatenate([e["J"] for e in ev], axis=1), cost=cost)
        e = eval_errors(got, ref, b, weighted_data(d, b))
        e["kappa"] = ev[0]["kappa"]
        out.append(e)
    return tuple(out)


def fp32_eval_bounds(gc):
    """fit_cases.fp32_eval_bounds over columns: per quantity FP32_UNIT_MARGIN x max(e_np32, eps32 kappa(W Phi)), both the
    largest over the case's distinct problems (the GPU tier holds the cost against it)"""
    e32 = numpy_evaluate_errors(gc, np.float32)
    floor = EPS32 * max(e["kappa"] for e in e32)
    return {k: FP32_UNIT_MARGIN * max(max(e[k] for e in e32), floor) for k in EVAL_KEYS}


def fp32_eval_bounds_per_problem(gc):
    """the same bound distinct problem by distinct problem (C, r and J)"""
    return [{k: FP32_UNIT_MARGIN * max(e[k], EPS32 * e["kappa"]) for k in EVAL_KEYS} for e in numpy_evaluate_errors(gc, np.float32)]


# ---- the reference algorithm in fp32 with several right-hand sides ---------------------------------------------------------
# oracle.lib_f32 is the oracle's source with fp32 storage; oracle.py binds its batched single-right-hand-side entry only.  The
# problem-level entries are in the library all the same (same names, float buffers), and they take S > 1.
class _Problem32(C.Structure):  # the head of vpo_problem (oracle/varpro_oracle.h) with `double` read as `float`
    _fields_ = [("model", O.ModelDesc), ("m", C.c_int), ("S", C.c_int), ("t", C.c_void_p), ("w", C.c_void_p), ("Yw", C.c_void_p),
                ("eps", C.c_float), ("alpha", C.POINTER(C.c_float))]


def fit_f32(model, x, Y, w, alpha0):
    """the oracle's global fit run in fp32 (fp32 default tolerances) on fp32 inputs x (m,), Y (S, m), w -> alpha (q,) fp32"""
    lib = O.lib_f32()
    fp = C.POINTER(C.c_float)
    lib.vpo_problem_create.restype = C.c_void_p
    lib.vpo_problem_create.argtypes = [C.POINTER(O.ModelDesc), C.c_int, C.c_int, fp, fp, fp, C.c_float, C.POINTER(C.c_int)]
    lib.vpo_set_params.argtypes = [C.c_void_p, fp]
    lib.vpo_set_params.restype = None
    lib.vpo_fit.argtypes = [C.c_void_p, C.POINTER(O.LmOpts), C.POINTER(O.Report)]
    lib.vpo_fit.restype = None
    lib.vpo_problem_destroy.argtypes = [C.c_void_p]
    lib.vpo_problem_destroy.restype = None
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    x, Y, w, a0 = f32(x), f32(Y), f32(w), f32(alpha0)
    desc, err = O.desc_of(model), C.c_int(0)
    h = lib.vpo_problem_create(C.byref(desc), Y.shape[1], Y.shape[0], O._fp(x), O._fp(Y), O._fp(w), -1.0, C.byref(err))
    assert h, "fp32 oracle problem build error %d" % err.value
    try:
        lib.vpo_set_params(h, O._fp(a0))
        opts, rep = O.default_opts_f32(), O.Report()
        lib.vpo_fit(h, C.byref(opts), C.byref(rep))
        st = C.cast(h, C.POINTER(_Problem32)).contents
        return np.array([st.alpha[i] for i in range(a0.size)], dtype=np.float32)
    finally:
        lib.vpo_problem_destroy(h)


@functools.lru_cache(maxsize=None)
def oracle_fit_f32_excess(gc):
    """(F(alpha_32) - F*) / F* per distinct problem for the reference algorithm run in fp32 from the case's guess: F the fp64
    oracle's cost over all columns, F* the objective of its own fit"""
    d, ref = case_data(gc), oracle_fit(gc)
    out = []
    for b in range(NB):
        x = d["x"] if d["x"].ndim == 1 else d["x"][b]
        w = None if d["w"] is None else (d["w"] if d["w"].ndim == 1 else d["w"][b])
        a32 = fit_f32(d["model"], x, d["Y"][b], w, d["guess"][b])
        out.append((oracle_cost(gc, b, a32) - ref["objective"][b]) / ref["objective"][b])
    return _ro(np.array(out))
