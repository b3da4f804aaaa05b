"""Cases and references of the per-kernel-set tests of the evaluation, the Kaufman Jacobian and the LM fit kernels
(tests/test_fit_cases_host.py, tests/test_gpu_fit_sets.py).

The set records, model shapes, the case record and its data are those of tests/stats_cases.py.  Here every case also names
the record of vp_debug_last_fit (kernel, padding, weighted, 0) it expects after a fit under set_fit_kernel("wave") and --
where the set has a slot kernel -- under "slots".  Per resident set of capacity 64 R W:

  A  m = 64 R W          uniform grid      no weights   the full variant (padding 1), the split evaluation kernel
  B  m = 64 R W - 1      non-uniform grid  no weights   odd m: element-wise loads; the last-pair variant (padding 2) for R > 2
  C  the set's smallest  uniform grid      shared w     the weighted instantiation (no slot kernel: "slots" reports the wave
     even m                                             kernel)
  D  m = 64 (R - 2) W    non-uniform grid  no weights   the last m of the general variant (padding 0); dropped where that m
                                                        belongs to a smaller set (every R = 2 set, me2o at R = 4)

then per-problem grids and weights (P), the length-agnostic sets (L), and the two generic sets (G).
References are computed once per case (functools.lru_cache) and returned read-only."""
import collections
import functools

import numpy as np

from oracle import oracle as O
from stats_cases import (B, EPS32, F32, F64, FP32_UNIT_MARGIN, PER_PROBLEM_CASES, SHAPES, blk_me_set, blk_rt_set, case, case_data,
                         case_id, fit_guess, gen_set, me_set, problem_inputs, rt_set)
from varpro_amd._lib import FAMILY_GENERIC, FAMILY_MULTIEXP

WAVE, SLOTS, GRAM, BLOCK, GENERIC = 1, 2, 3, 4, 5  # vp_debug_last_fit: kernel
FitCase = collections.namedtuple("FitCase", "cls case wave slots")


def fit_case_id(fc):
    return fc.cls + "-" + case_id(fc.case)


# ---- launch_fit's three inequalities, restated once ------------------------------------------------------------------------
def padding_class(m, R, W):
    """padding_variant (vp_fit.hpp), the one rule launch_fit and launch_fit2 pick their instantiation by length with for an
    UNWEIGHTED problem, restated: 1 if m == 64 R W; else 2 if R > 2 and m > 64 (R - 2) W; else 0"""
    if m == 64 * R * W:
        return 1
    if R > 2 and m > 64 * (R - 2) * W:
        return 2
    return 0


# ---- launch_fit2's LDS exit, restated once ----------------------------------------------------------------------------------
def slots_fit_lds(rec):
    """vp_fit2.hpp: a slot-kernel workgroup holds the shared grid and, for each of NG groups, at least one slot's data column
    of 64 R W elements, within its share 160 KiB / BPC of the CU's LDS (NG = 4 one-wave groups or one W-wave group; BPC from
    the resident waves per SIMD, waves_for: two where (N + P) R words-per-element <= 200 VGPRs, else one).  fit2_slots rounds
    a budget of less than one slot up to one, and launch_fit2 then leaves by its LDS exit.  Restated on the columns alone (the
    records and constants only add to it): no room when (1 + NG) columns already reach the share."""
    dtype, _fam, nexp, off, _c, R, W, _gen = rec
    size = 8 if dtype == F64 else 4
    ncols = (nexp + off) + nexp  # N + P of MultiExpModel: basis functions + derivative pairs
    wps = 2 if ncols * R * (size // 4) <= 200 else 1
    ng = 4 if W == 1 else 1
    bpc = max(1, (4 * wps) // (W * ng))
    return (1 + ng) * 64 * R * W * size < (160 * 1024) // bpc


def slot_launcher(rec):
    """launch_fit2 is a launcher of its own (not launch_fit under another name) for multi-exponential models that end in a
    constant column, on the Householder sets: not the fp32 Gram set, not the length-agnostic ones"""
    _dtype, fam, _a, b, _c, _R, _W, gen = rec
    return fam == FAMILY_MULTIEXP and b == 1 and not gen and not is_gram(rec)


def has_slot_kernel(rec):
    """... and it launches a slot kernel where a workgroup's slots fit the LDS.  ONE registered set has the launcher and no
    room: the single exponential + offset at 32 fp64 rows per lane (16 KiB per column, two workgroups per CU, five columns =
    80 KiB).  Its three slot kernels are built and never launched -- found by this table asking for the record.  What was
    chosen: the kernels and the launcher stay as they are (no code object of the library moves), the set STAYS in the slot
    tests, and what is asserted there is that "slots" reports the wave kernel; if the budget ever lets the slot kernel run, the
    expected record becomes (2, ...) by slots_fit_lds and the comparison with the wave kernel runs with it."""
    return slot_launcher(rec) and slots_fit_lds(rec)


def is_gram(rec):
    """fp32, several waves per problem: the fit runs on the Gram kernel (VP_REGISTER_MULTIEXP_W_GRAM)"""
    return rec[0] == F32 and rec[1] == FAMILY_MULTIEXP and rec[6] > 1 and not rec[7]


def expected_records(rec, m, weighted, per_problem=False):
    """(record under "wave", record under "slots" or None) of a fit of m rows on the set `rec`"""
    _dtype, fam, _a, _b, _c, R, W, gen = rec
    if fam == FAMILY_GENERIC:
        return (GENERIC, -1, int(weighted), 0), None
    if gen:
        return (BLOCK, -1, int(weighted), 0), None
    if is_gram(rec):  # (a ragged last group of four rows is masked through the weights: vp_fitg.hpp)
        return (GRAM, -1, int(weighted or m % 4 != 0), 0), None
    wave = (WAVE, 0 if weighted else padding_class(m, R, W), int(weighted), 0)
    if not slot_launcher(rec):
        return wave, None
    return wave, wave if (weighted or per_problem or not slots_fit_lds(rec)) else (SLOTS, padding_class(m, R, W), 0, 0)


# ---- the resident sets: shape -> (dtype, record maker, [(R, W), ...] in the order of their capacity) -------------------------
def _me(nexp, off, dtype=F64):
    return lambda R, W=1: me_set(dtype, nexp, off, R, W)


def _rt(n, q, p):
    return lambda R, W=1: rt_set(n, q, p, R, W)


RESIDENT = [
    ("me2o", F64, _me(2, 1), [(2, 1), (4, 1), (8, 1), (12, 1), (16, 1), (20, 1)]),
    ("me1o", F64, _me(1, 1), [(2, 1), (8, 1), (16, 1), (24, 1), (32, 1)]),
    ("me1", F64, _me(1, 0), [(2, 1), (16, 1)]),
    ("me2", F64, _me(2, 0), [(2, 1), (16, 1)]),
    ("me3o_wide", F64, _me(3, 1), [(2, 1), (8, 1), (16, 1), (20, 1), (8, 4)]),
    ("me3", F64, _me(3, 0), [(2, 1)]),
    ("me2o", F32, _me(2, 1, F32), [(2, 1), (8, 1), (16, 1)]),
    # (five exponentials a factor 4 apart at the large sizes; the four cases of <= 130 rows: see _inputs)
    ("me5o_wide", F32, _me(5, 1, F32), [(2, 1), (16, 4)]),
    ("rate1", F64, _rt(1, 1, 1), [(2, 1), (16, 1)]),
    ("rate1o", F64, _rt(2, 1, 1), [(2, 1), (16, 1)]),
    ("rate2", F64, _rt(2, 2, 2), [(2, 1), (16, 1)]),
    ("cos1", F64, _rt(1, 2, 2), [(2, 1), (16, 1)]),
    ("cos2", F64, _rt(2, 4, 4), [(2, 1), (16, 1)]),
    ("rate3", F64, _rt(3, 3, 3), [(2, 1), (16, 1)]),
    ("rate3o", F64, _rt(4, 3, 3), [(2, 1)]),
    ("cos_rate2", F64, _rt(3, 4, 4), [(2, 1)]),
    ("cos_rate2o", F64, _rt(4, 4, 4), [(2, 1)]),
    ("dexp_unit", F64, _rt(3, 2, 2), [(2, 1), (4, 1), (8, 1), (12, 1), (16, 1)]),
    ("oleary", F64, _rt(2, 3, 4), [(2, 1), (4, 1), (8, 1), (12, 1), (16, 1)]),
]
# stats_cases' m of the smallest set of a key; three rates + offset: at 100 weighted rows cond(H)^2 eps_longdouble = 1.3e-10 at
# one of the oracle's minima, over the cap of the CPU tier
SMALL_M = collections.defaultdict(lambda: 100, rate3o=102)


# Five exponentials + offset on <= 130 uniformly spaced rows are not determined at a relative noise of 1e-3
# (tools/fit_inputs_probe.py, profiles/fit_inputs_probe.json): the best scaled condition number kappa_s of H over 100 000 random
# sets of five decay times is 342 (128 rows) and 510 (100 rows), and of 293 spacings none lets the oracle fit more than 8 of the
# 20 problems of these four cases with the conditions of the CPU tier met (me5o_wide: terminations [4, -1, -1, 3, 3] at
# m = 128, [-1, -1, 3, -1, -1] at 127, [-4, -1, -1, -1, 4] at 100 weighted, [3, -1, 3, 4, -1] at 130 weighted).  The sizes are what
# reach the kernel variants, so THEY stay and the noise of these four cases goes down to 1e-5, with decay times a factor 3.2
# apart, which the few rows still sample: all twenty fits succeed there (19 of 20 at 1e-4).  Every other case keeps 1e-3.
def _inputs(shape, m):
    return dict(shape="me5o", noise=1e-5) if shape == "me5o_wide" and m <= 130 else dict(shape=shape)


def _case(shape, dtype, m, rec, **kw):
    kw.update(_inputs(shape, m))
    return case(dtype=dtype, m=m, kset=rec, **kw)


def _fc(cls, c, per_problem=False):
    wave, slots = expected_records(c.set, c.m, c.weights is not None, per_problem)
    return FitCase(cls, c, wave, slots)


def _resident_cases():
    out = []
    for shape, dtype, mk, sizes in RESIDENT:
        below = 0  # capacity of the next smaller set of the key
        for R, W in sizes:
            cap, rec = 64 * R * W, mk(R, W)
            out.append(_fc("A", _case(shape, dtype, cap, rec)))
            out.append(_fc("B", _case(shape, dtype, cap - 1, rec, uniform=False)))
            out.append(_fc("C", _case(shape, dtype, below + 2 if below else SMALL_M[shape], rec, weights="shared")))
            if 64 * (R - 2) * W > below:
                out.append(_fc("D", _case(shape, dtype, 64 * (R - 2) * W, rec, uniform=False)))
            below = cap
    return out


# ---- the length-agnostic sets: the first m past the largest resident set that takes the shape ------------------------------
# (a multi-exponential model without a resident set of its own at m runs on the run-time-descriptor set of its (n, q, p):
# find_kernels' second pass -- "me3" up to 1024 rows, "me4" up to 128)
STREAMED = [
    ("me2o", F64, 1281, blk_me_set(F64, 2, 1)), ("me1o", F64, 2049, blk_me_set(F64, 1, 1)), ("me1", F64, 1025, blk_me_set(F64, 1, 0)),
    ("me2", F64, 1025, blk_me_set(F64, 2, 0)), ("me3o_wide", F64, 2049, blk_me_set(F64, 3, 1)), ("me3", F64, 1025, blk_me_set(F64, 3, 0)),
    ("me4o", F64, 300, blk_me_set(F64, 4, 1)), ("me4", F64, 129, blk_me_set(F64, 4, 0)), ("me5o", F64, 300, blk_me_set(F64, 5, 1)),
    ("me5", F64, 300, blk_me_set(F64, 5, 0)), ("me2o", F32, 1025, blk_me_set(F32, 2, 1)), ("me5o_wide", F32, 4097, blk_me_set(F32, 5, 1)),
    ("rate1", F64, 1025, blk_rt_set(1, 1, 1)), ("rate1o", F64, 1025, blk_rt_set(2, 1, 1)), ("rate2", F64, 1025, blk_rt_set(2, 2, 2)),
    ("cos1", F64, 1025, blk_rt_set(1, 2, 2)), ("cos2", F64, 1025, blk_rt_set(2, 4, 4)), ("rate3", F64, 1025, blk_rt_set(3, 3, 3)),
    ("rate3o", F64, 129, blk_rt_set(4, 3, 3)), ("cos_rate2", F64, 129, blk_rt_set(3, 4, 4)), ("cos_rate2o", F64, 129, blk_rt_set(4, 4, 4)),
    ("dexp_unit", F64, 1025, blk_rt_set(3, 2, 2)), ("oleary", F64, 1025, blk_rt_set(2, 3, 4)),
]

RESIDENT_CASES = _resident_cases()
# (the triple exponential of the per-problem cases: the shape of the fit cases, see stats_cases.SHAPES)
PER_PROBLEM_FIT_CASES = [_fc("P", c._replace(shape="me3o_wide") if c.shape == "me3o" else c, per_problem=True) for c in PER_PROBLEM_CASES]
STREAMED_CASES = [_fc("L", case(shape, dtype, m, rec)) for shape, dtype, m, rec in STREAMED]
# (block height of the double exponential + offset in fp64: 8 rows per lane, 512 per block; 1290 = 2 * 512 + 266)
STREAMED_CASES.append(_fc("L", case("me2o", F64, 1290, blk_me_set(F64, 2, 1), stream=True, uniform=False)))
GENERIC_CASES = [_fc("G", case("mixed5", F64, 300, gen_set(F64), weights="shared")), _fc("G", case("mixed5", F32, 302, gen_set(F32)))]  # (at 300 rows one of the oracle's fp32-input fits ends where H is singular)
FIT_CASES = RESIDENT_CASES + PER_PROBLEM_FIT_CASES + STREAMED_CASES + GENERIC_CASES
IDS = [fit_case_id(fc) for fc in FIT_CASES]
# more problems than one wave's slots, for shapes other than the double exponential: the queue refill
REFILL_CASES = [fc for fc in RESIDENT_CASES if fc.cls == "A" and fc.case.set in (me_set(F64, 1, 1, 2), me_set(F64, 3, 1, 8, 4))]
REFILL_B = 700


def _ro(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def refill_data(c):
    """REFILL_B problems on the grid of a case: every problem its own decay times (the truth times 0.9 .. 1.1), coefficients
    and noise; guesses within 5 % of its decay times"""
    s, d = SHAPES[c.shape], case_data(c)
    rng = np.random.default_rng(REFILL_B + c.m)
    T = d["x"].dtype
    truth = np.asarray(s.truth) * rng.uniform(0.9, 1.1, (REFILL_B, len(s.truth)))
    coef = rng.uniform(5.0, 50.0, (REFILL_B, len(s.kinds)))
    Y = np.stack([coef[b] @ O.eval_phi(d["model"], d["x"], truth[b]) for b in range(REFILL_B)])
    Y = Y + c.noise * np.abs(Y).max(1, keepdims=True) * rng.standard_normal(Y.shape)
    guess = truth * rng.uniform(0.95, 1.05, truth.shape)
    return dict(model=d["model"], x=d["x"], Y=_ro(np.ascontiguousarray(Y, dtype=T)), guess=_ro(np.ascontiguousarray(guess, dtype=T)))


# ---- the library's criterion of a uniform grid -----------------------------------------------------------------------------
def grid_is_uniform(x):
    """grid_check_kernel (vp_api.hip), on a grid in the handle's dtype: with dt = (t[m-1] - t[0]) / (m - 1) finite and not
    zero, every |t[i] - fma(i, dt, t[0])| <= 4 eps(dtype) |t[i] - t[0]|, all in fp64; m >= 3"""
    x = np.asarray(x)
    eps = float(np.finfo(x.dtype).eps)
    t = x.astype(np.float64)
    m = t.size
    if m < 3:
        return False
    dt = (t[-1] - t[0]) / (m - 1)
    if not np.isfinite(dt) or dt == 0.0:
        return False
    lat = np.arange(m) * dt + t[0]  # (one rounding more than the fma: 1 ulp of t against a bound of 4 ulp of t - t[0] ...)
    dev = np.abs(t - lat)
    # ... so a grid is only CALLED uniform / non-uniform here when it is clear of the bound by a factor 2 either way
    tol = 4.0 * eps * np.abs(t - t[0])
    if (dev <= 0.5 * tol).all():
        return True
    assert (dev > 2.0 * tol).any(), "a grid within rounding of the library's bound: not a case for a test"
    return False


def handle_grid_uniform(c):
    d = case_data(c)
    return all(grid_is_uniform(g) for g in (d["x"] if d["x"].ndim == 2 else [d["x"]]))


# ---- references ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_fit(c):
    """the oracle's own fit of every problem from fit_guess, on the handle's inputs cast to fp64: dict(alpha (B, q), C (B, n),
    termination, n_evals, objective (B,), trace: list of (rows, q + 4))"""
    d, g = case_data(c), fit_guess(c)
    out = dict(alpha=[], C=[], termination=[], n_evals=[], objective=[], trace=[])
    for b in range(B):
        x, y, w = problem_inputs(d, b)
        p = O.Problem(d["model"], x, y, w=w)
        p.set_params(g[b].astype(np.float64))
        rep, tr = p.fit_trace(max_rows=16)
        out["alpha"].append(p.params())
        out["C"].append(p.linear_coefficients() if p.cached() else np.full(len(SHAPES[c.shape].kinds), np.nan))
        out["termination"].append(rep.termination)
        out["n_evals"].append(rep.n_evals)
        out["objective"].append(rep.objective)
        out["trace"].append(_ro(tr))
    return {k: (v if k == "trace" else _ro(np.array(v))) for k, v in out.items()}


def oracle_cost(c, b, alpha):
    """the variable projection functional 1/2 |r_w(alpha)|^2 of problem b, fp64 oracle"""
    d = case_data(c)
    x, y, w = problem_inputs(d, b)
    p = O.Problem(d["model"], x, y, w=w)
    p.set_params(np.asarray(alpha, dtype=np.float64))
    r = p.residuals()
    return np.inf if r is None else 0.5 * float(r @ r)


@functools.lru_cache(maxsize=None)
def oracle_evaluate(c):
    """O.evaluate_batch at the case's alpha on the handle's inputs cast to fp64, problem by problem (per-problem grids and
    weights included): dict(C (B, n), r (B, m), J (B, q, m), cost (B,), status (B,))"""
    d = case_data(c)
    parts = []
    for b in range(B):
        x, y, w = problem_inputs(d, b)
        parts.append(O.evaluate_batch(d["model"], x, y[None, :], d["alpha"][b:b + 1].astype(np.float64), w=w))
    return {k: _ro(np.concatenate([p[k] for p in parts])) for k in parts[0]}


def numpy_evaluate(model, x, y, w, alpha, dtype):
    """the evaluation restated in numpy by another route than the oracle's SVD, all arithmetic in `dtype` (the columns are
    evaluated in fp64 and rounded): W Phi = Q R; c = R^-1 Q^T y_w; r = y_w - W Phi c; J_k = -(v_k - Q Q^T v_k) with
    v_k = W D_k c.  -> dict(C, r, J (q, m), cost, wdc (q, m) = v_k, kappa = cond(W Phi) in fp64)"""
    T = np.dtype(dtype).type
    q = int(model.n_params)
    Phi = O.eval_phi(model, x, alpha).T
    wv = np.ones(x.size) if w is None else np.asarray(w, dtype=np.float64)
    kappa = float(np.linalg.cond(Phi * wv[:, None]))
    Pw = (np.ascontiguousarray(Phi, dtype=T) * wv.astype(T)[:, None]).astype(T)
    yw = (np.asarray(y, dtype=T) * wv.astype(T)).astype(T)
    Q, R = np.linalg.qr(Pw)
    cc = np.linalg.solve(R, Q.T @ yw)
    r = yw - Pw @ cc
    V = np.stack([(np.ascontiguousarray(O.eval_dphi(model, x, alpha, k).T, dtype=T) @ cc) * wv.astype(T) for k in range(q)])
    J = -(V - (Q @ (Q.T @ V.T)).T)
    out = dict(C=cc, r=r, J=J, cost=T(0.5) * T(r @ r), wdc=V)
    assert all(np.asarray(v).dtype == np.dtype(dtype) for v in out.values())
    out["kappa"] = kappa
    return out


EVAL_KEYS = ("C", "r", "J", "cost")


def eval_errors(got, ref, b, yw_max, yw_sq):
    """the metric of the evaluation comparison for problem b: C over max |C|, r over max |y_w|, J_k over max |J_k| (the
    largest over k), cost over max(cost, 1e-6 |y_w|^2) -- the scales of test_gpu_parity._check_eval"""
    g = {k: np.asarray(got[k], dtype=np.float64) for k in EVAL_KEYS}
    eJ = max(float(np.abs(g["J"][k] - ref["J"][b, k]).max() / np.abs(ref["J"][b, k]).max()) for k in range(ref["J"].shape[1]))
    return dict(C=float(np.abs(g["C"] - ref["C"][b]).max() / np.abs(ref["C"][b]).max()),
                r=float(np.abs(g["r"] - ref["r"][b]).max() / yw_max), J=eJ,
                cost=float(abs(g["cost"] - ref["cost"][b]) / max(ref["cost"][b], 1e-6 * yw_sq)))


@functools.lru_cache(maxsize=None)
def numpy_evaluate_errors(c, dtype):
    """per problem: the errors of numpy_evaluate run in `dtype` against the oracle, and cond(W Phi)"""
    d, ref = case_data(c), oracle_evaluate(c)
    out = []
    for b in range(B):
        x, y, w = problem_inputs(d, b)
        yw = y if w is None else y * w
        ev = numpy_evaluate(d["model"], x, y, w, d["alpha"][b].astype(np.float64), dtype)
        e = eval_errors(ev, ref, b, np.abs(yw).max(), float(yw @ yw))
        e["kappa"] = ev["kappa"]
        out.append(e)
    return tuple(out)


def fp32_eval_bounds(c):
    """fp32 sets: per quantity, FP32_UNIT_MARGIN x max(e_np32, eps32 kappa(W Phi)), e_np32 the error numpy's own fp32
    evaluation of the case makes.  Both the error and the bound are the largest over the case's five problems: one problem's
    fp32 error is one draw of the rounding (stats_cases.py on chi2), the case's largest is what a bound can be held against.
    (The GPU tier uses this for the cost and fp32_eval_bounds_per_problem for C, r and J.)"""
    e32 = numpy_evaluate_errors(c, np.float32)
    floor = EPS32 * max(e["kappa"] for e in e32)
    return {k: FP32_UNIT_MARGIN * max(max(e[k] for e in e32), floor) for k in EVAL_KEYS}


def fp32_eval_bounds_per_problem(c):
    """the same bound problem by problem: FP32_UNIT_MARGIN x max(e_np32 of that problem, eps32 kappa of that problem)"""
    return [{k: FP32_UNIT_MARGIN * max(e[k], EPS32 * e["kappa"]) for k in EVAL_KEYS} for e in numpy_evaluate_errors(c, np.float32)]


def device_ftol32():
    """the fp32 default ftol of vp_lm_opts_default"""
    import ctypes as C

    from varpro_amd import _lib
    o = _lib.LmOpts()
    _lib.load().vp_lm_opts_default(C.byref(o), F32)
    return float(o.ftol)


@functools.lru_cache(maxsize=None)
def oracle_fit_f32_excess(c):
    """(F(alpha_32) - F*) / F* per problem for O.fit_batch_f32, the reference algorithm run in fp32, from fit_guess: F the fp64
    oracle's cost, F* the objective of its own fit"""
    d, g, ref = case_data(c), fit_guess(c), oracle_fit(c)
    out = []
    for b in range(B):
        x = d["x"] if d["x"].ndim == 1 else d["x"][b]
        w = None if d["w"] is None else (d["w"] if d["w"].ndim == 1 else d["w"][b])
        a32, _C, _rep, _s = O.fit_batch_f32(d["model"], x, d["Y"][b:b + 1], g[b:b + 1], w=w)
        out.append((oracle_cost(c, b, a32[0]) - ref["objective"][b]) / ref["objective"][b])
    return _ro(np.array(out))

