/*
 * varpro_hip.h -- C ABI of the MI355X-native batched variable-projection hot path.
 *
 * This header is the drop-in boundary.  The reference
 * (geo-ant/varpro 0.13.3) has no FFI; its boundary is two Rust traits plus the
 * builder/solver facade.  Every entry point below cites the reference item whose
 * observable contract it replaces (paths relative to the reference repository).
 * A Rust shim (bindings/rust/) implements
 * `SeparableNonlinearModel` / `LeastSquaresProblem` on top of these calls.
 *
 * Conventions (the reference's own, src/lib.rs:42-87):
 *   m  number of observations                  model.output_len()          src/model/mod.rs:263
 *   n  number of basis functions               base_function_count()       src/model/mod.rs:259
 *   q  number of nonlinear parameters alpha    parameter_count()           src/model/mod.rs:256
 *   S  number of right-hand sides              Y_w.ncols()                 src/solvers/levmar/mod.rs:111
 *   B  batch of independent problems (new; the reference solves one problem per call)
 *
 * Memory layouts (row index fastest == nalgebra column-major per problem):
 *   t      [m]  (shared)   or [B][m]  with VP_FLAG_T_PER_PROBLEM
 *   w      [m]  (shared)   or [B][m]  with VP_FLAG_W_PER_PROBLEM, NULL => Weights::Unit
 *   Y, R   [B][S][m]       residual vector of problem b == vec(R_b) (src/util/mod.rs:101-106)
 *   alpha  [B][q]
 *   C      [B][S][n]
 *   J      [B][q][S][m]    problem b: (m*S) x q column-major, RHS s at rows s*m.. (src/solvers/levmar/mod.rs:147-153)
 *   Phi    [B][n][m]       dPhi [B][p][m], p = number of (basis,param) dependency pairs in model order
 *
 * All data pointers of one handle live in one address space chosen at creation:
 * host (default; the library stages through hipMemcpyAsync) or device
 * (VP_FLAG_DEVICE_PTRS; zero copies, everything enqueued on the handle's stream).
 * One handle <-> one HIP stream; handles are independent and re-entrant, there is
 * no global state (the reference is single-threaded and Clone, src/problem.rs:55).
 *
 * Return value of every call: 0 = ok, <0 = call-level error (vp_last_error()).
 * Per-problem failures never abort a batch; they are latched in status[b]
 * exactly like `cached = None` in the reference (src/solvers/levmar/mod.rs:61-72):
 * status[b] != 0  <=>  residuals()/jacobian() would return None for problem b.
 */
#ifndef VARPRO_HIP_H
#define VARPRO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VP_MAX_BASIS 8        /* n <= 8 */
#define VP_MAX_PARAMS 8       /* q <= 8 */
#define VP_MAX_BASIS_PARAMS 2 /* parameters one basis function may depend on */
#define VP_MAX_PAIRS 16       /* p <= 16 non-zero (basis,param) derivative columns */

/* scalar type of the problem == SeparableNonlinearModel::ScalarType (src/model/mod.rs:246) */
enum { VP_F64 = 0, VP_F32 = 1 };

/*
 * Closed descriptor language for basis functions.  The reference
 * accepts opaque Rust closures (src/model/model_basis_function.rs:11-12) which
 * cannot run on a GPU; these kinds cover every model the reference's tests and
 * benches use.  kind -> f(t, p0[, p1]) and its partial derivatives:
 */
enum {
    VP_BASIS_CONST = 0,     /* 1                       invariant_function, shared_test_code/src/lib.rs:123     */
    VP_BASIS_EXP_DECAY = 1, /* exp(-t/p0)              d/dp0 = exp(-t/p0)*t/p0^2   shared_test_code/src/lib.rs:101-114 */
    VP_BASIS_EXP_RATE = 2,  /* exp(-p0*t)              d/dp0 = -t*exp(-p0*t)                                    */
    VP_BASIS_EXP_COS = 3,   /* exp(-p0*t)*cos(p1*t)    d/dp0 = -t*f ; d/dp1 = -t*exp(-p0*t)*sin(p1*t)
                               shared_test_code/src/models.rs:310-372 (O'Leary example)                         */
    VP_BASIS_SIN_PHASE = 4, /* sin(p0*t+p1)            d/dp0 = t*cos(p0*t+p1) ; d/dp1 = cos(p0*t+p1)
                               src/test_helpers/mod.rs:28-52                                                     */
    VP_BASIS_EXTERNAL = 5,  /* evaluated by the CALLER: any SeparableNonlinearModel (src/model/mod.rs:239-363), in
                               particular the closure-based SeparableModel (:441-512).  Only produced by
                               vp_batch_create_external; see "models outside the descriptor language" below          */
    /* peak and baseline kinds, d = t - p0 (see "device-column handles" below) */
    VP_BASIS_GAUSS = 6,     /* exp(-d^2/(2 p1^2))      d/dp0 = f*d/p1^2 ; d/dp1 = f*d^2/p1^3                            */
    VP_BASIS_LORENTZ = 7,   /* p1^2/(d^2 + p1^2)       d/dp0 = 2 p1^2 d/(d^2 + p1^2)^2 ; d/dp1 = 2 p1 d^2/(d^2 + p1^2)^2 */
    VP_BASIS_LINEAR = 8,    /* t                       invariant_function (no parameters): a sloped baseline            */
    /* IRF reconvolution kinds (see "IRF reconvolution" below): the handle's instrument response irf (vp_set_irf) on a UNIFORM
     * grid of step dt, rho = exp(-dt/p0).  Rectangle rule: lag 0 included, NO factor dt (the linear coefficient absorbs it) */
    VP_BASIS_EXP_DECAY_IRF = 9, /* sum_{k<=i} irf_k rho^(i-k)     d/dp0 = dt/p0^2 sum_{k<=i} (i-k) rho^(i-k) irf_k
                                   i.e. F_i = irf_i + rho F_{i-1}, H_i = rho (H_{i-1} + F_{i-1}), d/dp0 = dt/p0^2 H_i      */
    VP_BASIS_IRF = 10,          /* irf_i                   invariant (no parameters): the scattered-light term             */
    /* kind 9 with the response repeating every period T = P dt, P >= m real (see "Periodic IRF reconvolution" below):
     * sum_{p>=0} sum_k irf_k rho^(i-k+pP) over the terms with i-k+pP >= 0; the same recurrence from a non-zero start   */
    VP_BASIS_EXP_DECAY_IRF_PERIODIC = 11,
    /* kinds 9 - 11 on the response SHIFTED by delta, a fit parameter (see "Shifted IRF reconvolution" below): g_i = r(i - s),
     * s = delta/dt, r the Catmull-Rom cubic through the samples, zero outside the record; g' = dg/ddelta                  */
    VP_BASIS_EXP_DECAY_IRF_SHIFT = 12, /* p0 = tau, p1 = delta: kind 9 on g; d/dp0 as kind 9, d/dp1 = kind 9's Phi on g'   */
    VP_BASIS_IRF_SHIFT = 13,           /* p0 = delta: g_i; d/dp0 = g'_i   (the scattered-light term, shifted)              */
    VP_BASIS_EXP_DECAY_IRF_PERIODIC_SHIFT = 14 /* p0 = tau, p1 = delta: kind 11 on g (the period of vp_set_irf_period);
                                                  d/dp1 = kind 11's Phi on g'                                              */
};

/*
 * Device-column handles.  A descriptor that contains at least one of VP_BASIS_GAUSS / VP_BASIS_LORENTZ / VP_BASIS_LINEAR
 * (next to any of the kinds 0..4) makes vp_batch_create build a DEVICE-COLUMN handle: one kernel (vp_cols.hpp) evaluates
 * the unweighted columns Phi [B][n][m] and dPhi [B][p][m] of ALL its basis functions into two buffers the handle owns --
 * B*n*m and B*p*m elements of the handle's dtype, allocated at the first call that needs them -- and the kernels of
 * caller-evaluated models (below) do everything downstream, exactly as they do for a caller's columns.  A descriptor of
 * the kinds 0..4 alone takes the in-register kernels as before -- unless the handle is created with
 * VP_FLAG_DEVICE_COLUMNS, which makes a device-column handle of any descriptor (the column kernel evaluates all eight
 * kinds), e.g. to bound the decay times of a multi-exponential fit.  On a device-column handle
 *   vp_set_params, vp_evaluate, vp_basis, vp_residuals, vp_jacobian, vp_linear_coeffs, vp_cost, vp_params, vp_best_fit,
 *   vp_statistics, vp_global_statistics, vp_weighted_data, vp_set_observations, vp_summary*, vp_reduce_cost work as on any
 *   descriptor handle (shared and per-problem grids, weights, any S, both dtypes; m < n included);
 *   vp_fit  runs the stepped LM of vp_fit_begin / _step_with_basis / _end inside the library: per step one launch of the
 *           column kernel over the still-active problems (the step kernel's compacted list, read on the device) and one
 *           step launch; the host looks at the active count every 8 steps.  Afterwards the handle's state is the fitted
 *           point INCLUDING its columns: vp_residuals, vp_jacobian, vp_best_fit and the statistics need no further call.
 *           m < n: VP_ERR_UNSUPPORTED (as for vp_fit_begin);
 *   VP_ERR_UNSUPPORTED: vp_set_params_with_basis, vp_jacobian_with_derivatives, vp_evaluate_with_basis, vp_fit_begin,
 *           vp_fit_step_with_basis, vp_fit_active_set, vp_fit_end (the handle is not caller-evaluated), vp_fit_trace,
 *           vp_set_rhs_allreduce (as on caller-evaluated handles), vp_debug_gram_evaluate;
 *   vp_set_fit_kernel, VP_FLAG_STREAM_ROWS and VP_FLAG_NO_GRID_RECURRENCE are accepted and have no effect;
 *   vp_set_bounds  puts box bounds on the nonlinear parameters of vp_fit (only device-column handles take them).  A bounded
 *           fit is a smooth re-parameterisation alpha = g(u) in the manner of MINUIT / lmfit -- per parameter
 *               lo and hi:  alpha = lo + (hi - lo)/2 (sin u + 1)      lo only:  alpha = lo - 1 + sqrt(u^2 + 1)
 *               hi only:    alpha = hi + 1 - sqrt(u^2 + 1)            neither:  alpha = u
 *           -- and the unchanged LM drivers iterate on u: vp_fit maps alpha0 to u (a guess outside the box is clamped
 *           onto it first), a bounded variant of the column kernel evaluates the model at g(u) and scales the derivative
 *           columns by dalpha/du, and the result is mapped back.  Every returned parameter lies inside its box, bounds
 *           included, exactly (the value is clamped after g; fp32 handles round the box inwards).  The returned alpha is,
 *           bit for bit, the point at which the handle's final columns were evaluated, so vp_params, vp_residuals,
 *           vp_jacobian, vp_best_fit, vp_statistics and vp_global_statistics are in the caller's parameters and need no
 *           further call, as after any fit.  To know:
 *             - ftol / xtol / gtol act on u, as in lmfit;
 *             - a start ON a bound stays on it (dalpha/du = 0 there): start strictly inside the box;
 *             - the statistics of a parameter that ends on a bound are those of the unconstrained linearisation at that
 *               point (they do not know about the bound);
 *             - bounds constrain vp_fit only: vp_set_params, vp_evaluate and vp_basis take alpha as given, unclipped.
 *
 * IRF reconvolution.  A descriptor that contains VP_BASIS_EXP_DECAY_IRF or VP_BASIS_IRF makes a device-column handle as
 * well: measured decays (fluorescence lifetimes, ring-down traces) are sum_j c_j exp(-t/tau_j) CONVOLVED with the instrument
 * response, and "iterative reconvolution" fits exactly this model.  The columns of these two kinds come from a scan kernel of
 * their own (vp_irf.hpp: one wavefront per problem and function), every other kind of the same descriptor from the column
 * kernel as before; a model such as c1 (irf * exp tau1) + c2 (irf * exp tau2) + c3 irf + c4, or a mix with a Gaussian, is
 * one descriptor.  Such a handle needs its response before anything that needs columns: until vp_set_irf has been called,
 * vp_set_params, vp_evaluate, vp_basis, vp_fit and vp_search answer VP_ERR_INVALID (and the statistics "no parameters set
 * yet").  The grid must be UNIFORM, shared or per problem: dt_b = (t_b[m-1] - t_b[0]) / (m-1); m = 1 is allowed (the column
 * is irf_0, the derivative 0).  Host-pointer grids are checked at creation -- |t_i - t_0 - i dt| <= 1e-6 |dt|, else
 * VP_ERR_INVALID; for device-pointer grids (VP_FLAG_DEVICE_PTRS) uniformity is the CALLER'S CONTRACT: the kernel uses the
 * two end points only.  tau <= 0, a NaN tau or a non-finite response entry give non-finite columns, latched per problem
 * like every other non-finite Phi.  Bounds, vp_search and the statistics work as on any device-column handle (a response
 * per problem sends vp_search down its candidate loop, like a grid per problem).
 *
 * Periodic IRF reconvolution.  VP_BASIS_EXP_DECAY_IRF assumes the decay is zero before the record starts (F_{-1} = 0).  With
 * a pulsed laser whose period T is not long against tau, the remainder exp(-T/tau) of every earlier pulse's decay lies under
 * the record ("incomplete decays").  VP_BASIS_EXP_DECAY_IRF_PERIODIC = 11 is the steady state of that pulse train: one
 * parameter tau, uniform grids only, rectangle rule, lag 0 included, no factor dt -- like kind 9.  The response is taken as
 * zero outside the record and repeats with period T in the units of the grid; P = T/dt bins, real, P >= m; rho = exp(-dt/tau):
 *     Phi_i      = sum_{p>=0} sum_k irf_k rho^(i-k+pP)   (terms with i-k+pP >= 0)   = F_i^lin + rho^(i+1) F_{-1}
 *     dPhi_i/dtau = (dt/tau^2) H_i,   H_i = H_i^lin + rho^(i+1) (H_{-1} + (i+1) F_{-1})
 * i.e. the recurrence of kind 9, F_i = irf_i + rho F_{i-1}, H_i = rho (H_{i-1} + F_{i-1}), started from
 *     A = F^lin_{m-1}, B = H^lin_{m-1}                  (the totals of the zero-start recurrence at row m-1)
 *     g = P - m (bins), e = exp(-(T - m dt)/tau)        (exactly 1 when g = 0)
 *     E = exp(-T/tau),  D = -expm1(-T/tau)
 *     F_{-1} = e A / D,   H_{-1} = (e/D) (g A + B + P E A / D)
 * The period belongs to the handle (vp_set_irf_period): 0, the default, means that the record is exactly one period,
 * T = m dt_b per grid (g = 0, e = 1 exactly); otherwise T = period for the whole batch.  Host-pointer grids are checked:
 * period < m dt_b (1 - 1e-6) on any grid is VP_ERR_INVALID; within that band g is taken as 0.  Device-pointer grids are the
 * caller's contract: g < -1e-6 m gives NaN columns, latched per problem like tau <= 0.  A descriptor with this kind needs
 * m >= 2 (m = 1: dt = 0, the periodic sum diverges) -- creation answers VP_ERR_INVALID -- and may mix kinds 9, 10 and 11.
 *
 * Shifted IRF reconvolution.  A measured response is recorded at another wavelength or count rate than the decay and sits a
 * fraction of a bin to a few bins away from where the decay's rising edge wants it.  The kinds 12 - 14 are the kinds 9 - 11
 * on the response shifted by delta, a nonlinear parameter like any other (bounds, fixing, vp_search, the statistics).  The
 * grid is uniform with step dt as for kind 9; delta is in the units of the grid, s = delta/dt in bins, and a POSITIVE delta
 * moves the response to LATER times.  The response is ZERO OUTSIDE THE RECORD: nothing wraps, not for the periodic kind
 * either -- this suits responses that are negligible at the record's edges.  g_i = r(i - s), with r the Catmull-Rom cubic
 * through the samples:
 *     o = floor(-s),  f = -s - o  in [0,1)                                   (both uniform over the problem)
 *     g_i              =         sum_{a=-1..2} w_a(f)  irf_{i+o+a}
 *     dg_i/ddelta = g'_i = -(1/dt) sum_{a=-1..2} w'_a(f) irf_{i+o+a}
 *     w_-1  = (-f^3+2f^2-f)/2    w_0  = (3f^3-5f^2+2)/2    w_1  = (-3f^3+4f^2+f)/2    w_2  = (f^3-f^2)/2
 *     w'_-1 = (-3f^2+4f-1)/2     w'_0 = (9f^2-10f)/2       w'_1 = (-9f^2+8f+1)/2      w'_2 = (3f^2-2f)/2
 * (sum w = 1, sum w' = 0; g' is continuous across integer shifts, so the Jacobian has no jumps -- which is why the
 * interpolant is cubic and not linear; f = 0 gives w = (0, 1, 0, 0) exactly: delta = 0 reproduces the response bit for bit,
 * an integer shift moves its samples exactly, zeros shifted in).  Because the recurrences of kinds 9 and 11, and the
 * steady-state carry of kind 11, are linear in the response, every column of a shifted kind is an existing scan over g or g':
 *     12 (tau, delta):  Phi, d/dtau = kind 9 on g;   d/ddelta = the Phi recurrence of kind 9 on g'
 *     13 (delta):       Phi = g;                     d/ddelta = g'
 *     14 (tau, delta):  Phi, d/dtau = kind 11 on g;  d/ddelta = kind 11's Phi on g'
 * One resample kernel (vp_irf_shift.hpp) writes g and g' per problem into two buffers the handle owns -- [B][ms] each, ms = m
 * rounded up to a 16-byte group, 2 B ms elements of the handle's dtype, allocated at the first call that needs columns -- and
 * the scan kernels of kinds 9 - 11 run over them, unchanged.  Under vp_set_bounds delta = g(u) like every parameter (g' is
 * multiplied by ddelta/du in the resample kernel); on a vp_batch_create_fixed handle a fixed delta is read per problem from
 * the fixed values and has no derivative column.  Rules:
 *   - all functions of kinds 12 - 14 of one descriptor name the SAME delta parameter (one response, one shift), and no
 *     function of another kind -- nor the tau of a shifted function -- may be that parameter: else VP_ERR_INVALID at creation;
 *   - m >= 2 (dt = 0 otherwise): VP_ERR_INVALID at creation, as for kind 11;
 *   - a non-finite s gives NaN columns, latched per problem like tau <= 0; |s| >= m + 2 gives exact zeros in g and g';
 *   - kinds 9 - 11 may stand next to 12 - 14 in one descriptor: they keep reading the handle's own, unshifted response;
 *   - vp_set_irf, vp_set_irf_period (kind 14 counts as periodic), vp_basis into caller arrays, S > 1, both dtypes, grids
 *     and responses per problem work as for kinds 9 - 11; vp_search on such a handle takes its candidate loop (as for a
 *     response per problem), because g belongs to the problem, not to the candidate.
 *
 * Parameters for which Phi is not finite (a NaN guess; p1 = 0 with p0 on a grid point: 0 / 0) are latched per problem in
 * status[b], like a caller's non-finite columns; p1 = 0 elsewhere gives a finite Phi (exp(-inf) = 0) whose Gaussian
 * derivatives are NaN -- a fit from there ends VP_TERM_NUMERICAL, as the reference's does.  The batch is never aborted.
 */

/*
 * Model descriptor == what SeparableModelBuilder::build() produces
 * (src/model/builder/mod.rs:338-525): basis functions in insertion order
 * (column j of Phi == basis j, src/model/builder/mod.rs:512-515) and, per basis
 * function, which entries of alpha it depends on (the "Ind" table of
 * matlab/examples/adaex.m:33-34; src/model/detail.rs:60-127).
 * param[j][a] = index into alpha of argument a of basis j, or -1 if unused.
 */
typedef struct vp_model_desc {
    int32_t n_basis;  /* n */
    int32_t n_params; /* q */
    int32_t kind[VP_MAX_BASIS];
    int32_t param[VP_MAX_BASIS][VP_MAX_BASIS_PARAMS];
} vp_model_desc;

/* creation flags */
enum {
    VP_FLAG_DEVICE_PTRS = 1 << 0,   /* every data pointer passed for this handle is a device pointer */
    VP_FLAG_T_PER_PROBLEM = 1 << 1, /* t is [B][m] instead of [m] */
    VP_FLAG_W_PER_PROBLEM = 1 << 2, /* w is [B][m] instead of [m] */
    VP_FLAG_OWN_STREAM = 1 << 3,    /* ignore hip_stream and run on a private non-blocking stream */
    /* fp64 kernels evaluate exp(-t/tau) on a grid that is uniform to rounding (checked once at creation:
     * |t_i - (t_0 + i dt)| <= 4 eps |t_i - t_0|) by a per-lane recurrence instead of one exponential per row;
     * results then agree with the per-row form to ~1e-15 relative instead of 1 ulp.  This flag keeps the per-row
     * exponential (== the reference's evaluation, shared_test_code/src/lib.rs:101-114) regardless of the grid. */
    VP_FLAG_NO_GRID_RECURRENCE = 1 << 4,
    /* Single-RHS fits of this handle run on the LENGTH-AGNOSTIC kernels (rows streamed in blocks through a TSQR-style
     * update of an (n+1+p)^2 triangle; any m) even where a register-resident kernel set covers m.  The library selects them
     * by itself beyond the largest resident set; the flag exists for memory-lean handles and for the parity tests.  Ignored
     * for models without such a set (they run on the generic kernels, as before). */
    VP_FLAG_STREAM_ROWS = 1 << 5,
    /* A descriptor of the kinds 0..4 alone becomes a DEVICE-COLUMN handle too (see "device-column handles" above): its
     * columns go through device memory instead of registers -- slower than the in-register kernels, but such a handle
     * takes vp_set_bounds.  No effect on descriptors with a peak / baseline kind (they are device-column handles anyway)
     * and on vp_batch_create_external. */
    VP_FLAG_DEVICE_COLUMNS = 1 << 6
};

/* per-problem status word (0 == the reference's `cached = Some(..)`) */
enum {
    VP_ST_OK = 0,
    VP_ST_NONFINITE = 1,    /* Phi, C or R contains inf/nan (model error / SVD solve error path) */
    VP_ST_NOT_EVALUATED = 2 /* residuals()/jacobian() before any set_params() */
};

/* call-level error codes */
enum {
    VP_ERR_OK = 0,
    VP_ERR_INVALID = -1,     /* bad handle / argument / shape (builder errors, src/problem/builder.rs:15-46) */
    VP_ERR_UNSUPPORTED = -2, /* operation not available for this handle.  Every MODEL the descriptor can express is
                              * accepted for every entry point -- shapes without a specialised kernel set run on generic
                              * kernels, global fits (S > 1) and any batch size included; m < n (an underdetermined
                              * linear sub-problem) takes the reference's minimum-norm solution; right-hand-side sharding
                              * (vp_set_rhs_allreduce) works on every shape.  What remains unsupported: vp_statistics with
                              * S > 1 (as in the reference; vp_global_statistics covers global fits), vp_global_statistics
                              * of sharded right-hand sides, vp_debug_gram_evaluate on handles without the Gram kernel */
    VP_ERR_HIP = -3,         /* HIP runtime failure */
    VP_ERR_NO_DEVICE = -4    /* no gfx950 device / library built without device code */
};

/* builder validation errors mirror SeparableProblemBuilderError (src/problem/builder.rs:15-46);
 * returned by vp_batch_create as VP_ERR_INVALID with one of these in vp_last_error_detail() */
enum {
    VP_BUILD_OK = 0,
    VP_BUILD_Y_DATA_MISSING = 1,
    VP_BUILD_INVALID_LENGTH_OF_DATA = 2,
    VP_BUILD_ZERO_LENGTH_VECTOR = 3,
    VP_BUILD_INVALID_PARAMETER_COUNT = 4,
    VP_BUILD_INVALID_LENGTH_OF_WEIGHTS = 5
};

/*
 * LM driver options == levenberg_marquardt::LevenbergMarquardt builder knobs
 * reached through LevMarSolver::with_solver (src/solvers/levmar/mod.rs:221-223).
 * Defaults (vp_lm_opts_default): ftol = xtol = gtol = 30*eps(dtype), stepbound = 100,
 * patience = 100 (max evaluations = patience*(q+1)), scale_diag = 1.
 */
typedef struct vp_lm_opts {
    double ftol;
    double xtol;
    double gtol;
    double stepbound;
    int32_t patience;
    int32_t scale_diag;
} vp_lm_opts;

/* termination == levenberg_marquardt::TerminationReason; >0 <=> was_successful()
 * (src/fit.rs:120-122, src/solvers/levmar/mod.rs:249-253) */
enum {
    VP_TERM_RESIDUALS_ZERO = 1,
    VP_TERM_ORTHOGONAL = 2,
    VP_TERM_CONVERGED_FTOL = 3,
    VP_TERM_CONVERGED_XTOL = 4,
    VP_TERM_CONVERGED_BOTH = 5,
    VP_TERM_NOT_RUN = 0,
    VP_TERM_USER = -1, /* residuals()/jacobian() returned None */
    VP_TERM_NUMERICAL = -2,
    VP_TERM_NO_IMPROVEMENT = -3,
    VP_TERM_LOST_PATIENCE = -4,
    VP_TERM_NO_PARAMETERS = -5,
    VP_TERM_NO_RESIDUALS = -6,
    VP_TERM_WRONG_DIMENSIONS = -7
};

/* == levenberg_marquardt::MinimizationReport (src/fit.rs:24-29) */
typedef struct vp_report {
    int32_t termination;
    int32_t n_evals;  /* number_of_evaluations */
    double objective; /* objective_function = 1/2 ||r||^2 */
} vp_report;

typedef struct vp_batch vp_batch;

/* ---- lifetime ------------------------------------------------------------------------- */

/*
 * == SeparableProblemBuilder::{new|mrhs, observations, weights, epsilon, build}
 * (src/problem/builder.rs:116,194,142,220,261,246,278-324) for B problems at once.
 * Validates shapes, stores Y_w = W*Y (src/problem/builder.rs:307), default epsilon
 * = machine epsilon of dtype when svd_epsilon < 0 (src/problem/builder.rs:282).
 * Unlike build() it does NOT run the initial set_params (there is no alpha yet);
 * vp_set_params / vp_fit do.  `hip_stream` is the hipStream_t all work of this handle is
 * enqueued on; NULL means the HIP null (default) stream -- which is what PyTorch's default
 * stream is -- unless VP_FLAG_OWN_STREAM asks for a private stream.
 */
int vp_batch_create(vp_batch **h, const vp_model_desc *model, int dtype, int64_t m, int64_t S, int64_t B,
                    const void *t, const void *Y, const void *w, double svd_epsilon, int flags, int device,
                    void *hip_stream);

/* == Drop of SeparableProblem */
void vp_batch_destroy(vp_batch *h);

/* ---- LeastSquaresProblem surface (src/solvers/levmar/mod.rs:22-202) --------------------- */

/*
 * == SeparableProblem::set_params (src/solvers/levmar/mod.rs:42-73) incl.
 * model.set_params/eval (src/model/mod.rs:266-267,308) and the weighting
 * (src/util/weights.rs:82-99): Phi_w = W Phi(alpha); solve min ||Y_w - Phi_w C||
 * with singular values <= epsilon truncated; R = Y_w - Phi_w C.  Caches C, R,
 * 1/2||R||^2 and status per problem (== CachedCalculations, src/problem.rs:88-107).
 */
int vp_set_params(vp_batch *h, const void *alpha);

/* == LeastSquaresProblem::params (src/solvers/levmar/mod.rs:80-82) */
int vp_params(vp_batch *h, void *alpha_out);

/* == LeastSquaresProblem::residuals (src/solvers/levmar/mod.rs:91-95): r_b = vec(R_b).
 * status may be NULL. */
int vp_residuals(vp_batch *h, void *r_out, int32_t *status);

/* == LeastSquaresProblem::jacobian (src/solvers/levmar/mod.rs:101-201): Kaufman
 * Jacobian J[:,k] = -vec(P_perp W dPhi/dalpha_k C), incl. eval_partial_deriv
 * (src/model/mod.rs:359-362).  status may be NULL. */
int vp_jacobian(vp_batch *h, void *J_out, int32_t *status);

/* == SeparableProblem::linear_coefficients (src/problem.rs:142-147,173-183) */
int vp_linear_coeffs(vp_batch *h, void *C_out, int32_t *status);

/* == SeparableProblem::weighted_data (src/problem.rs:154-156,189-196) */
int vp_weighted_data(vp_batch *h, void *Yw_out);

/*
 * Replace the observations of an existing handle (same B, S, m, model, grid and weights): Y_w = W*Y is recomputed on
 * the handle's stream and every cached result is invalidated.  The batch counterpart of building a new
 * SeparableProblem with SeparableProblemBuilder::observations (src/problem/builder.rs:219-232) for the next frame
 * of a stream of same-shaped data, without re-allocating the device state.  Y is [B][S][m] like at creation
 * (host or device pointer according to the handle's flags).
 */
int vp_set_observations(vp_batch *h, const void *Y);

/*
 * Replace the weights of a handle that was CREATED WITH weights (same B, S, m, model and grid).  w has the layout fixed at
 * creation -- [m], or [B][m] with VP_FLAG_W_PER_PROBLEM -- and the handle's dtype and address space.  Y [B][S][m] must be
 * passed again: the handle keeps only Y_w = W*Y (vp_batch_create), not Y, so the new weighted data can only be formed from
 * the caller's observations.  Every cached evaluation / fit is invalidated, as by vp_set_observations; afterwards the handle
 * is, bit for bit, the handle vp_batch_create would have made with these weights.  Any S and every handle kind (in-register,
 * device-column, caller-evaluated) is accepted.  Device-pointer handles stay asynchronous (one copy, one launch).
 * VP_ERR_INVALID: a null pointer, a stepped fit in progress, a handle created without weights (w == NULL selected the
 * kernel set of Weights::Unit at creation; such a handle cannot take weights later).  VP_ERR_UNSUPPORTED: a handle padded
 * for m < n.  A refusal leaves the handle as it was.
 */
int vp_set_weights(vp_batch *h, const void *w, const void *Y);

/*
 * Poisson-weighted fits.  Photon counts y_i are Poisson with mean f_i, so the weight of a least-squares fit is
 * w_i = 1/sqrt(variance_i).  vp_poisson_reweight forms the weights ON THE DEVICE, replaces the handle's weights and its
 * weighted data by them -- one pass (vp_poisson.hpp) -- and the next vp_fit uses them:
 *   VP_POISSON_NEYMAN   variance = max(y_i, floor)   from the counts Y alone ("Neyman" weighting)
 *   VP_POISSON_MODEL    variance = max(f_i, floor)   from the handle's current best fit f = Phi(alpha) c, UNWEIGHTED, as
 *                       vp_best_fit returns it ("Pearson" / model weighting), evaluated into a [B][m] scratch buffer the
 *                       handle owns (allocated at the first call).  Needs parameters (after vp_fit, vp_set_params,
 *                       vp_evaluate, vp_search or -- caller-evaluated handles -- vp_set_params_with_basis, whose columns
 *                       must still be valid).  Works on in-register, device-column and caller-evaluated handles.
 *   w_i = 1/sqrt(variance_i),  Y_w,i = w_i y_i       floor > 0 keeps empty bins finite; 1 is customary
 *   deviance_out [B] f64   D   = 2 sum_i [ y_i ln(y_i/ft_i) - (y_i - ft_i) ],  ft = max(f, floor); the logarithmic term is 0
 *                              for y_i <= 0: the Poisson deviance, the goodness-of-fit number of a likelihood fit
 *   pearson_out  [B] f64   X^2 = sum_i (y_i - ft_i)^2 / ft_i
 *                          both of the fit the weights were formed FROM, accumulated in double for both dtypes in a fixed
 *                          order; they follow the handle's address space, either may be NULL, and both MUST be NULL in Neyman
 *                          mode (there is no fit to judge).
 * A fit with w = 1/sqrt(f) held fixed, f re-formed from the result and the fit repeated from the previous parameters has as
 * its fixed point the Poisson score equations sum_i (y_i - f_i)/f_i df_i/dtheta = 0: iterating {vp_poisson_reweight(MODEL),
 * vp_fit} IS the Poisson maximum-likelihood fit (the first round weighted by VP_POISSON_NEYMAN).  A fixed number of rounds
 * keeps a device-pointer pipeline free of host visits (measured: DESIGN.md section 3i).
 * A problem whose status is non-zero in model mode (its evaluation failed, there is no fit) keeps its weights and weighted
 * data and gets NaN in both sums: a failed round does not poison the next one.  A non-finite count or fit value gives a
 * non-finite weight, and the next evaluation latches the problem like any other non-finite input.
 * Afterwards every cached evaluation is invalidated (the residuals belong to the old weights); vp_params still returns the
 * parameters, so that the next vp_fit can start from them.  Device-pointer handles stay asynchronous, except for the one
 * allocation of the scratch buffer at the first model-mode call.
 * To know:
 *   - vp_statistics after the last round is the statistics of the WEIGHTED LEAST-SQUARES problem at the final weights: with
 *     w = 1/sqrt(f) that is the Fisher-information covariance at the maximum-likelihood estimate, the usual one; its
 *     reduced chi^2 is Pearson's X^2 / (m - n - q) at the weights of the previous round, not the deviance;
 *   - bounds (vp_set_bounds), vp_search and vp_set_irf compose unchanged: they act on the fit, not on the weights;
 *   - weights are per problem, not per right-hand side: S = 1 only; this is iterated re-weighting, not an LM on deviance
 *     residuals; m < n is not covered.
 * VP_ERR_INVALID: a null Y, an unknown mode, a floor that is not finite and > 0, outputs passed in Neyman mode, a stepped fit
 * in progress, a handle not created with VP_FLAG_W_PER_PROBLEM and a weights array, model mode before any parameters are set
 * and -- caller-evaluated handles -- model mode without columns at the current parameters.  VP_ERR_UNSUPPORTED: S > 1, a
 * handle padded for m < n.  A refusal leaves the handle as it was.
 */
enum { VP_POISSON_NEYMAN = 0, VP_POISSON_MODEL = 1 };
int vp_poisson_reweight(vp_batch *h, const void *Y, int mode, double floor,
                        double *deviance_out, double *pearson_out);

/*
 * Robust fits.  Measured data has outliers (afterpulses, stray-light and cosmic-ray spikes, hot channels); an M-estimator
 * replaces the square of a residual by a loss rho that grows more slowly.  vp_robust_reweight forms the weights of the
 * equivalent weighted least-squares problem ON THE DEVICE from the residuals of the handle's current best fit
 * f = Phi(alpha) c (UNWEIGHTED, as vp_best_fit returns it), replaces the handle's weights and weighted data by them
 * (vp_robust.hpp), and the next vp_fit uses them:
 *   e_i = w0_i (y_i - f_i)             w0 [B][m]: the BASE weights, in the handle's dtype and address space; NULL: 1.  They
 *                                      should make the residuals of the clean data homoscedastic (1/sigma_i; Neyman weights
 *                                      for counts).  The handle's own weights are overwritten every round, so -- like Y --
 *                                      the base weights are passed again each time.
 *   s                                  scale > 0: that value for the whole batch (rounded to the handle's dtype; the choice
 *                                      when w0 = 1/sigma is known).  scale == 0: per problem the normalised median of the
 *                                      absolute residuals, s = 1.482602218505602 med, med = 0.5 (a[(me-1)/2] + a[me/2]) of
 *                                      the sorted |e_i| over the me rows with w0_i != 0 (rows of weight 0 are how a ragged
 *                                      length is expressed and do not pull the median down), selected exactly.  A problem
 *                                      with s == 0 (me == 0 included) gets w = w0, Y_w = w0 y, scale 0 and rho 0.
 *   u_i = e_i / s,  t = |u|/k          k = tuning; 0 selects the 95 %-efficiency constant: 1.345, 2.385, 4.685
 *   VP_ROBUST_HUBER    omega = 1 for |u| <= k, else k/|u|;      rho = u^2/2, or k|u| - k^2/2 beyond k
 *   VP_ROBUST_CAUCHY   omega = 1/(1 + t^2);                     rho = (k^2/2) log1p(t^2)
 *   VP_ROBUST_TUKEY    sqrt(omega) = (1 - t)(1 + t), 0 for t >= 1;   rho = (k^2/6)(1 - (1 - t^2)^3), k^2/6 beyond
 *   w_i = w0_i sqrt(omega_i),  Y_w,i = w_i y_i
 *   scale_out [B] f64   s as used;  rho_out [B] f64   sum_i rho(u_i), accumulated in double in a fixed order.  Either may be
 *                       NULL; both follow the handle's address space.
 * A fit with these weights held fixed, the weights re-formed from its result and the fit repeated from the previous
 * parameters has as its fixed point the estimating equations sum_i psi(u_i) w0_i df_i/dtheta = 0, psi = u omega: iterating
 * {vp_robust_reweight, vp_fit} IS the M-estimate (iterated re-weighting, not a Levenberg-Marquardt on rho).  Cauchy and
 * Tukey are not convex: start them from a sensible fit.  vp_statistics afterwards is the covariance of the weighted
 * least-squares problem at the final weights, not a sandwich estimator.
 * Preconditions and what follows are those of VP_POISSON_MODEL: parameters at which the handle can form its best fit,
 * a handle created with VP_FLAG_W_PER_PROBLEM and a weights array, S = 1, no padding for m < n, no stepped fit running;
 * afterwards cached evaluations are invalid, vp_params still returns the parameters, and a device-pointer handle has made
 * no host visit.  A problem whose status is non-zero keeps its weights and weighted data bit for bit and gets NaN in both
 * outputs.  A residual that is not finite gives NaN weights (scale == 0: the whole problem, with a NaN scale; scale > 0:
 * that row), so that the next evaluation latches the problem.
 * VP_ERR_INVALID: null Y, an unknown loss, a tuning or scale that is negative or not finite, and what VP_POISSON_MODEL
 * refuses with that code.  VP_ERR_UNSUPPORTED: S > 1, a handle padded for m < n.  A refusal leaves the handle as it was.
 */
enum { VP_ROBUST_HUBER = 0, VP_ROBUST_CAUCHY = 1, VP_ROBUST_TUKEY = 2 };
int vp_robust_reweight(vp_batch *h, const void *Y, const void *w0, int loss, double tuning, double scale,
                       double *scale_out, double *rho_out);
/* the handle's current weights, [m] or [B][m] as created, into w_out (a copy on the handle's stream; after
 * vp_robust_reweight they are the outlier map of the fit).  VP_ERR_INVALID on a handle created without weights. */
int vp_weights(vp_batch *h, void *w_out);

/* Box bounds on the nonlinear parameters of vp_fit, device-column handles only (see "device-column handles" above).
 * lower / upper: HOST pointers to doubles whatever the handle's dtype and flags, [q] (per_problem = 0) or [B][q];
 * -INFINITY / +INFINITY = unbounded on that side; both NULL clears the bounds.  Stays set across vp_fit calls and
 * vp_set_observations.
 * VP_ERR_INVALID: a NaN, lower >= upper (a parameter is fixed at creation: vp_batch_create_fixed), exactly one pointer
 * NULL, a stepped fit in progress.  VP_ERR_UNSUPPORTED: not a device-column handle (create it with
 * VP_FLAG_DEVICE_COLUMNS).  A refusal leaves the handle, and the bounds it had, as they were. */
int vp_set_bounds(vp_batch *h, const double *lower, const double *upper, int per_problem);

/*
 * Fixed nonlinear parameters: "this parameter is known, do not fit it" (lmfit's vary=False, the "fix tau2" box of FLIM
 * programs, a peak width set to the instrument's resolution).
 *
 * vp_batch_create_fixed takes everything vp_batch_create takes, plus
 *   fixed        [q] int32, 0 (free) or 1 (fixed) per parameter of the descriptor;
 *   values       [q] (per_problem = 0) or [B][q] DOUBLES whatever the handle's dtype, a host or device pointer according to
 *                VP_FLAG_DEVICE_PTRS; entries of free parameters are ignored.  The handle copies them (on its stream);
 *   per_problem  0: one set of values for the batch, 1: one per problem.
 * It builds a device-column handle of ANY descriptor of the device kinds (kinds 0..4 alone become one as well, as under
 * VP_FLAG_DEVICE_COLUMNS), and THE HANDLE IS THE REDUCED MODEL: from creation on every entry point sees a model of q_free
 * parameters, the free ones in the descriptor's order -- vp_set_params, vp_evaluate, vp_fit, vp_params, vp_jacobian, vp_basis
 * (dPhi: the pairs of free parameters only, in model order), vp_search (candidates [K][q_free]), vp_set_bounds ([q_free]
 * boxes; they compose), vp_statistics / vp_global_statistics (cov [q_free][q_free]: the covariance of the problem that was
 * solved) and the info queries.  Only the column kernels know the full parameter vector; the fit writes and factors fewer
 * derivative columns.  A function whose parameters are all fixed has no derivative column and behaves like an invariant one.
 * A mask of zeros is legal: an ordinary device-column handle in everything observable.
 * A fixed value at which a column is not finite (a width 0, tau <= 0, a NaN) is NOT refused -- values may live on the device --
 * and gives NaN columns, latched for that problem alone as for a parameter of that value.
 * VP_ERR_INVALID: what vp_batch_create refuses, a null mask, a mask entry other than 0 or 1, every parameter fixed (no free
 * parameter left; a descriptor without parameters and its empty mask are legal), null values when any parameter is fixed.  VP_ERR_UNSUPPORTED: a caller-evaluated descriptor (VP_BASIS_EXTERNAL).
 *
 * vp_set_fixed_values replaces the values between fits (same mask, same layout rules; copied on the handle's stream): the
 * next point of a profile-likelihood scan.  Every cached evaluation / fit is invalidated.  VP_ERR_INVALID: null values on a
 * handle with a fixed parameter.  VP_ERR_UNSUPPORTED: a handle that was not created by vp_batch_create_fixed.  The mask cannot
 * change after creation.  (A stepped fit cannot be in progress on such a handle: vp_fit_begin refuses device-column handles.)
 */
int vp_batch_create_fixed(vp_batch **out, const vp_model_desc *model, int dtype, int64_t m, int64_t S, int64_t B, const void *t,
                          const void *Y, const void *w, double svd_epsilon, int flags, int device, void *hip_stream,
                          const int32_t *fixed, const double *values, int per_problem);
int vp_set_fixed_values(vp_batch *h, const double *values, int per_problem);

/* The instrument response of a handle whose descriptor contains VP_BASIS_EXP_DECAY_IRF / VP_BASIS_IRF (see "IRF
 * reconvolution" above).  irf: [m] (per_problem = 0) or [B][m], the handle's dtype, a host or device pointer according to
 * VP_FLAG_DEVICE_PTRS; the handle COPIES it into a buffer it owns (on its stream; device pointers: no synchronisation).  May
 * be called again to replace the response (the next frame of a stream, with vp_set_observations); every cached evaluation /
 * fit is invalidated.  VP_ERR_INVALID: null irf, a handle without these kinds, a stepped fit in progress. */
int vp_set_irf(vp_batch *h, const void *irf, int per_problem);

/* The period T of VP_BASIS_EXP_DECAY_IRF_PERIODIC in the units of the grid, shared by the batch (see "Periodic IRF
 * reconvolution" above).  0 (the default): the record is exactly one period, T = m dt_b per grid.  Every cached evaluation /
 * fit is invalidated, as by vp_set_irf.  VP_ERR_INVALID: a handle whose model has no periodic kind, a NaN or negative period,
 * a stepped fit in progress, and -- host-pointer grids -- period < m dt_b (1 - 1e-6) on any grid. */
int vp_set_irf_period(vp_batch *h, double period);

/*
 * Start-point search: rank K candidate parameter vectors per problem ON THE DEVICE and leave the best one in the handle.
 * Every fit starts from a guess (vp_fit's alpha_inout; the reference's initial parameters, src/problem/builder.rs:116); with
 * variable projection only the q nonlinear parameters need one, and the value of a guess is the projected objective
 * 1/2 ||P_perp(alpha) y_w||^2 -- what vp_cost returns after vp_set_params(alpha).
 *   cand       the handle's dtype and address space; [K][q] shared by all problems (flags = 0) or [B][K][q] with
 *              VP_SEARCH_PER_PROBLEM; K >= 1
 *   alpha_out  [B][q]  per problem the candidate with the smallest 1/2 ||vec R_b||^2 (summed over the S right-hand sides)
 *   index_out  [B]     its index; ties go to the lowest index among the candidates that are equal in the device's arithmetic
 *   cost_out   [B] f64 the cost of the EVALUATION at the winner (below), not the ranking score: it has vp_evaluate's accuracy,
 *                      not that of a difference of squares
 * Each output may be NULL.  Afterwards the handle's state is exactly that of vp_set_params(h, alpha_out): vp_params,
 * vp_linear_coeffs, vp_residuals, vp_cost and status refer to the winners.
 * Candidates whose Phi is not finite (a NaN; sigma = 0 on a grid point) never win while another candidate of the problem is
 * finite.  A problem without a finite candidate gets index_out = -1 and its candidate 0 in alpha_out, and its status is
 * latched non-zero as by vp_set_params.  The batch is never aborted.  Bounds (vp_set_bounds) are not consulted: candidates
 * are taken as given, as in vp_set_params.
 * Two routes.  Candidates, grid and weights shared by the batch (and m >= n): the K bases are factored once -- the column
 * kernel evaluates the candidates, one workgroup each orthonormalises their weighted columns (a direction whose remainder
 * is <= 64 eps of its column's norm is dropped: the score of the minimum-norm solution) -- and the ranking is ONE matrix
 * product (B S x m)(m x K n) with the running maximum of sum_j (q_kj . y_w)^2 in its epilogue, then one evaluation at the
 * winners (measured: DESIGN.md section 3g).  Anything per problem (candidates, grid, weights) and m < n: K cost-only
 * evaluations through the handle's own kernels with a running minimum on the device, then the evaluation at the winners.
 * "Not finite" is decided by the ELEMENTS of W Phi on both routes: the shared route scales a column by its largest
 * magnitude before it squares anything, so a finite column of any size is ranked.
 * Device-pointer handles stay asynchronous on both routes, with one exception: the scratch of the shared route is sized by
 * K and grown on demand -- the FIRST call, and any call with a larger K (or a first call with S > 1), allocates, and
 * replacing a smaller block frees it, which synchronises the device.  Calls with the same or a smaller K enqueue only.
 * Every descriptor handle is accepted (in-register and device-column, both dtypes, any S, any m).
 * VP_ERR_INVALID: null cand, K < 1, an unknown flag, a stepped fit in progress.  VP_ERR_UNSUPPORTED: a caller-evaluated
 * handle (the device cannot evaluate the model), right-hand sides sharded over ranks (vp_set_rhs_allreduce).  A refusal
 * leaves the handle as it was.
 */
enum { VP_SEARCH_PER_PROBLEM = 1 };
int vp_search(vp_batch *h, const void *cand, int64_t K, int flags,
              void *alpha_out, int32_t *index_out, double *cost_out);

/* 1/2 ||vec R_b||^2 per problem, always f64 [B] (== MinimizationReport::objective_function) */
int vp_cost(vp_batch *h, double *cost_out);

/*
 * Fused evaluation: set_params + any subset of {residuals, jacobian, coefficients,
 * cost} in ONE kernel launch with Phi never leaving the chip.  NULL outputs are
 * skipped.  Equivalent to the sequence of calls above (same cached state after).
 */
int vp_evaluate(vp_batch *h, const void *alpha, void *r_out, void *J_out, void *C_out, double *cost_out,
                int32_t *status);

/* ---- model surface -------------------------------------------------------------------- */

/*
 * == SeparableNonlinearModel::{set_params, eval, eval_partial_deriv}
 * (src/model/mod.rs:266-267,308,359-362) for the whole batch, UNWEIGHTED:
 * Phi_out[b][j][:] = basis j; dPhi_out[b][pair][:] = d basis_j / d alpha_k for the
 * dependency pairs in model order (basis-major).  Either output may be NULL.
 * flags: VP_BASIS_SKIP_INVARIANT omits VP_BASIS_CONST columns from Phi_out (then
 * Phi_out is [B][n_alpha][m]); this is the stand-alone Phi kernel whose HBM
 * roofline fraction BASELINE.json asks for.
 */
enum { VP_BASIS_SKIP_INVARIANT = 1 };
int vp_basis(vp_batch *h, const void *alpha, void *Phi_out, void *dPhi_out, int flags);

/* ---- models outside the descriptor language --------------------------------
 *
 * The reference's plugin boundary is a TRAIT: any `SeparableNonlinearModel` (src/model/mod.rs:239-363) works with its
 * solver -- the closure-based `SeparableModel` (src/model/mod.rs:441-512, src/model/model_basis_function.rs:11-28) and
 * every hand-written impl (shared_test_code/src/models.rs:40-150).  A model the closed descriptor language above cannot
 * express (a pseudo-Voigt or any other basis function of three parameters, a table look-up, ...) crosses this ABI as
 * the VALUES the trait returns: the caller evaluates `eval()` -> Phi and `eval_partial_deriv(k)` -> its non-zero
 * columns; the device does everything downstream of them -- weighting (src/solvers/levmar/mod.rs:47,141), the
 * factorisation / truncated solve / residual (:51-59) and the Kaufman Jacobian (:101-201).
 *
 * vp_batch_create_external == SeparableProblemBuilder::{new|mrhs, observations, weights, epsilon, build}
 * (src/problem/builder.rs:116-324) for a model that is known by its SHAPE only:
 *   n_basis, n_params   base_function_count() / parameter_count()                   src/model/mod.rs:256-259
 *   n_pairs, pair_basis[], pair_param[]
 *                       the (basis j, parameter k) pairs with d phi_j / d alpha_k != 0, i.e. the columns
 *                       eval_partial_deriv(k) does not leave zero (src/model/mod.rs:473-512; the "Ind" table of
 *                       matlab/examples/adaex.m:33-34).  Any order, each pair once, n_pairs <= VP_MAX_PAIRS.  A basis
 *                       function may depend on ANY number of parameters (no VP_MAX_BASIS_PARAMS limit here), and a
 *                       caller that does not know the sparsity lists all n*q pairs.
 * There is no grid: the independent variable is the caller's business (src/model/mod.rs:441-471 captures it in the
 * closures).  Y, w, svd_epsilon, flags (VP_FLAG_DEVICE_PTRS, VP_FLAG_W_PER_PROBLEM, VP_FLAG_OWN_STREAM), device and
 * hip_stream as for vp_batch_create.
 *
 * On such a handle:
 *   vp_set_params_with_basis   == SeparableProblem::set_params (src/solvers/levmar/mod.rs:42-73) with the model call at
 *                              :43-45 (`model.set_params(alpha); model.eval()`) replaced by its result:
 *                                Phi   [B][n][m]         UNWEIGHTED basis matrix of every problem (column j = basis j)
 *                                dPhi  [B][n_pairs][m]   UNWEIGHTED d phi_j / d alpha_k for the pairs in table order, or
 *                                                        NULL (derivatives follow with vp_jacobian_with_derivatives --
 *                                                        the LM driver asks for a Jacobian only at accepted points)
 *                              alpha is stored (vp_params) but not interpreted.  Caches C, R, cost, status like
 *                              vp_set_params.  Host-pointer handles copy Phi / dPhi; device-pointer handles keep the
 *                              POINTERS: the arrays must stay valid and unchanged until the next vp_set_params_with_basis
 *                              / vp_evaluate_with_basis / vp_batch_destroy (the model owns its matrices in the
 *                              reference, too).
 *   vp_jacobian_with_derivatives == SeparableProblem::jacobian (:101-201) with `model.eval_partial_deriv(k)` (:141)
 *                              replaced by its non-zero columns dPhi [B][n_pairs][m] at the current parameters.
 *   vp_evaluate_with_basis     the fused form (== vp_evaluate): Phi, dPhi in -> any subset of r, J, C, cost, status out in
 *                              one pass over the columns.  dPhi may be NULL when J_out is.
 *   vp_residuals, vp_jacobian (needs the dPhi of the last vp_set_params_with_basis), vp_linear_coeffs, vp_cost,
 *   vp_params, vp_weighted_data, vp_set_observations, vp_best_fit, vp_statistics, vp_synchronize work as on any handle.
 *   vp_set_params / vp_evaluate / vp_basis / vp_fit: VP_ERR_UNSUPPORTED -- the device cannot evaluate the model.  A FIT
 *   of such a batch runs by reverse communication: vp_fit_begin / vp_fit_step_with_basis / vp_fit_end below (the
 *   device keeps the LM loop, the caller keeps the model); one LM driver per problem on the host over the trait-level
 *   entries above (tests/c/test_external_model.c drives one) remains possible.
 */
int vp_batch_create_external(vp_batch **h, int32_t n_basis, int32_t n_params, int32_t n_pairs, const int32_t *pair_basis,
                             const int32_t *pair_param, int dtype, int64_t m, int64_t S, int64_t B, const void *Y,
                             const void *w, double svd_epsilon, int flags, int device, void *hip_stream);
int vp_set_params_with_basis(vp_batch *h, const void *alpha, const void *Phi, const void *dPhi);
int vp_jacobian_with_derivatives(vp_batch *h, const void *dPhi, void *J_out, int32_t *status);
int vp_evaluate_with_basis(vp_batch *h, const void *alpha, const void *Phi, const void *dPhi, void *r_out, void *J_out,
                           void *C_out, double *cost_out, int32_t *status);

/* ---- solver surface ------------------------------------------------------------------- */

void vp_lm_opts_default(vp_lm_opts *opts, int dtype);

/*
 * == LevMarSolver::fit (src/solvers/levmar/mod.rs:238-254) -> LevenbergMarquardt::minimize (call site :247) for a BATCH of
 * problems whose model only the caller can evaluate -- any SeparableNonlinearModel (src/model/mod.rs:239-363) on a handle
 * made by vp_batch_create_external -- by REVERSE COMMUNICATION.  The reference's driver talks to the problem through three
 * trait calls: set_params(x_trial) (:42-73, which evaluates the model, :43-45), residuals() (:91-95) and, at accepted
 * points only, jacobian() (:101-201, which asks the model for eval_partial_deriv(k), :141).  Here the device keeps the
 * whole driver -- one LM record per problem: trust region, lmpar, accept / reject, the crate's termination tests -- and
 * the model's answers cross the boundary as arrays; what comes back per step is alpha_trial [B][q] and one word per
 * problem.  Neither the residuals nor the Jacobian J [B][q][m] are ever written to memory.
 *
 *   vp_fit_begin(h, opts, alpha0, flags)
 *       starts a fit of all B problems from alpha0 [B][q] (opts == NULL: vp_lm_opts_default).  The first step takes the
 *       columns at alpha0.  flags: 0, or VP_FIT_DERIVATIVES_ON_ACCEPT (below).
 *   vp_fit_step_with_basis(h, Phi, dPhi, alpha_trial_out, want_out, n_active_out)
 *       Phi  [B][n][m], dPhi [B][n_pairs][m]: UNWEIGHTED model columns at the trial points the previous step returned
 *       (alpha0 for the first step), laid out as for vp_set_params_with_basis.  One launch runs, for every problem still
 *       active, one LM iteration: the evaluation at the trial point, the accept / reject decision and termination tests,
 *       at an accepted point the pivoted QR of the Kaufman Jacobian, and the next trust-region step.  Outputs (any may
 *       be NULL; same address space as the handle's other arrays):
 *         alpha_trial_out [B][q]  where the columns are wanted next; for a finished problem its final parameters
 *         want_out        [B]     VP_WANT_BASIS | VP_WANT_DERIVATIVES bits, 0 = the problem has terminated.  Entries of
 *                                 Phi / dPhi of problems that do not want them are never read.
 *         n_active_out    host    number of problems still running (reading it synchronises the handle's stream; pass
 *                                 NULL to keep a device-pointer pipeline asynchronous and look every few steps)
 *       Default protocol: every step carries Phi AND dPhi (want is 3 or 0) and is one LM iteration of every problem.
 *       VP_FIT_DERIVATIVES_ON_ACCEPT: the driver's own call order -- trial points want Phi only (want = 1, dPhi is not
 *       read and may be NULL); a problem that ACCEPTS its trial point answers want = 3 with the same alpha_trial and
 *       forms its Jacobian from the columns of the next step.  eval_partial_deriv is then evaluated exactly where the
 *       reference evaluates it, at the price of a second pass over Phi per accepted point.  A problem whose want = 3
 *       request is answered with dPhi == NULL ends with VP_TERM_USER (the reference: eval_partial_deriv failed ->
 *       jacobian() == None); a handle WITHOUT dependency pairs (n_pairs == 0: every eval_partial_deriv is zero) never
 *       reads dPhi and its fits end `Orthogonal` at alpha0 -- the zero Jacobian's scaled gradient is 0 <= gtol.
 *   vp_fit_end(h, alpha_out, C_out, rep)
 *       FitResult::nonlinear_parameters / linear_coefficients (src/fit.rs:113-115) and the MinimizationReport of every
 *       problem (rep[b].termination == VP_TERM_NOT_RUN for a problem the caller stopped stepping before it terminated;
 *       its best point so far is returned).  Afterwards the handle holds alpha, C, cost and status of the fitted point
 *       (vp_params, vp_linear_coeffs, vp_cost, vp_summary*, vp_reduce_cost); entries that need the MODEL at that point
 *       (vp_residuals, vp_jacobian, vp_best_fit, vp_statistics) first need its columns: vp_set_params_with_basis.
 * Every problem terminates after at most patience*(q+1) evaluations (TerminationReason::LostPatience), so stepping until
 * n_active == 0 always ends.  Covered: EVERY shape vp_batch_create_external admits -- n <= VP_MAX_BASIS, q <= VP_MAX_PARAMS,
 * any pair table, any number of right-hand sides S (fit<Rhs>, src/problem/builder.rs:194-225: the S data columns share
 * alpha, the residual is the stacked one, C_out of vp_fit_end is [B][S][n]) -- at ANY m >= n: the (n, q, pairs) of the
 * compiled step kernels register-resident to 4 096 rows and streamed in row blocks beyond (shapes of up to ten columns
 * n + 1 + pairs), every other shape and every S > 1 on the generic step kernel.  m < n: VP_ERR_UNSUPPORTED.
 */
enum { VP_FIT_DERIVATIVES_ON_ACCEPT = 1 };
enum { VP_WANT_BASIS = 1, VP_WANT_DERIVATIVES = 2 };
int vp_fit_begin(vp_batch *h, const vp_lm_opts *opts, const void *alpha0, int flags);
int vp_fit_step_with_basis(vp_batch *h, const void *Phi, const void *dPhi, void *alpha_trial_out, int32_t *want_out,
                           int64_t *n_active_out);
int vp_fit_end(vp_batch *h, void *alpha_out, void *C_out, vp_report *rep);
/*
 * The ACTIVE SET of the running fit, compacted: after a step, index_out[0 .. *count_out) are the problems still running
 * (want != 0), in no particular order; entries beyond the count are valid problem indices of finished problems (stale, never
 * out of range).  A model that evaluates only these -- instead of scanning want_out [B] -- does work proportional to the
 * problems left: the tail of a batched fit is a few hundred problems for ~100 steps (the reference's driver runs each of
 * them alone, src/solvers/levmar/mod.rs:247).  The device's own evaluation launch already covers just this set.  Both
 * arrays follow the handle's address space (device pointers: two asynchronous copies, no synchronisation; index_out [B]).
 */
int vp_fit_active_set(vp_batch *h, int32_t *index_out, int32_t *count_out);

/*
 * == LevMarSolver::fit (src/solvers/levmar/mod.rs:238-254), i.e.
 * LevenbergMarquardt::minimize (third-party, call site :247) for every problem of
 * the batch, device-resident.  alpha_inout: in = initial guess (the problem's
 * current params), out = FitResult::nonlinear_parameters (src/fit.rs:113-115).
 * C_out (may be NULL) = FitResult::linear_coefficients.  rep[b] (may be NULL) =
 * MinimizationReport; rep[b].termination > 0 <=> fit returned Ok.  After the call
 * the handle's cached state corresponds to the final parameters.
 */
int vp_fit(vp_batch *h, const vp_lm_opts *opts, void *alpha_inout, void *C_out, vp_report *rep);

/*
 * Diagnostics for the per-iteration parity tests: vp_fit that additionally
 * records, per problem, one row [alpha_trial(q), ||r(alpha_trial)||, ratio, delta, par] for every
 * evaluation of the LM loop (row 0: the initial point, ratio = NaN) into
 * trace_out [B][trace_rows][q+4] (f64; rows never written are NaN).  Same address space as the
 * other pointers of the handle.
 */
int vp_fit_trace(vp_batch *h, const vp_lm_opts *opts, void *alpha_inout, void *C_out, vp_report *rep,
                 double *trace_out, int trace_rows);

/* == FitResult::best_fit (src/fit.rs:55-59,87-91): UNWEIGHTED Phi(alpha) * C, [B][S][m] */
int vp_best_fit(vp_batch *h, void *fit_out);

/*
 * == FitStatistics::try_calculate (src/statistics/mod.rs:352-441) for every problem of a single-RHS batch at
 * the handle's current parameters (after vp_fit / vp_set_params); what fit_with_statistics
 * (src/solvers/levmar/mod.rs:275-304) adds to fit.
 *   cov_out            [B][(n+q)][(n+q)]  sigma^2 (H^T H)^-1, H = W [Phi, (dPhi/dalpha_k c)_k]; ordering
 *                      [linear coefficients, nonlinear parameters] (covariance_matrix(), :129)
 *   reduced_chi2_out   [B] f64            ||r_w||^2 / (m - n - q)  (reduced_chi2(), :183)
 *   conf_sigma_out     [B][m] or NULL     sqrt(j_i^T Cov j_i): multiply by the Student-t quantile
 *                                         t_ppf((p+1)/2, m-n-q) to get confidence_band_radius(p) (:271-304)
 *   status             [B] or NULL        0 ok; 4 = Underdetermined / MatrixInversion (the reference's Err)
 */
int vp_statistics(vp_batch *h, void *cov_out, double *reduced_chi2_out, void *conf_sigma_out, int32_t *status);

/*
 * Fit statistics of a GLOBAL fit (one alpha shared by the S right-hand sides of a problem, any S >= 1): the open item
 * "Fit statistics (and confidence bands, but also correlation matrix etc) for problems with multiple RHS" of the
 * reference's Todo.md, answered by FitStatistics::try_calculate (src/statistics/mod.rs:352-441) applied unchanged to the
 * equivalent single-RHS problem: observations vec(Y) (m S rows, stacked weights), parameters [c_1 .. c_S, alpha]
 * (n S + q), model (I_S (x) Phi(alpha)) vec(C).  Nothing of size (n S + q)^2 is formed: Phi_w = QR,
 * the Schur complement M of H^T H on the alpha block is the Gram matrix of the Kaufman Jacobian, factored in double.
 * At the handle's current parameters (after vp_fit, vp_set_params, vp_set_params_with_basis or -- with the columns of the
 * fitted point passed by vp_set_params_with_basis -- vp_fit_end); descriptor and caller-evaluated handles alike.
 *   cov_alpha_out       [B][q][q]       handle dtype   sigma^2 M^-1 = Cov(alpha, alpha)
 *   reduced_chi2_out    [B] f64                        sum_s ||r_w,s||^2 / (m S - n S - q)
 *   coef_cov_out        [B][S][n][n] or NULL           Cov(c_s, c_s)
 *   coef_alpha_cov_out  [B][S][n][q] or NULL           Cov(c_s, alpha)  (row a = coefficient a)
 *   conf_sigma_out      [B][S][m] or NULL              sqrt(j_{s,i}^T Cov j_{s,i}) with the UNweighted rows: multiply by
 *                                                      t_ppf((p+1)/2, m S - n S - q) for the confidence band radius
 *   status              [B] or NULL                    0 ok; 4 = Underdetermined / MatrixInversion of the stacked problem
 *                                                      (m S <= n S + q, a zero / non-finite pivot of R or of M, or an
 *                                                      evaluation that was not ok); its outputs are NaN
 * The cross blocks Cov(c_s, c_t), s != t, are not produced.  With S == 1 the outputs are vp_statistics' blocks.
 * Errors: VP_ERR_INVALID -- no parameters set yet, a null cov_alpha_out / reduced_chi2_out, or (caller-evaluated handle)
 * no Phi / dPhi at the current parameters; VP_ERR_UNSUPPORTED -- right-hand sides sharded over ranks
 * (vp_set_rhs_allreduce: the statistics need sums over ALL right-hand sides, a cross-rank reduction this entry does not
 * make), or a shape beyond n <= 8, q <= 8, n_pairs <= 16.
 */
int vp_global_statistics(vp_batch *h, void *cov_alpha_out, double *reduced_chi2_out, void *coef_cov_out,
                         void *coef_alpha_cov_out, void *conf_sigma_out, int32_t *status);

/*
 * Local batch aggregates for the multi-GPU cost reduction:
 * out = { sum_b 1/2||r_b||^2 , #successful , #failed , sum_b n_evals } over this
 * handle's problems (after vp_fit) -- always HOST doubles.  The cross-rank sum is one
 * RCCL all-reduce of these 4 doubles, issued by the host layer.
 */
int vp_summary(vp_batch *h, double out[4]);

/* Conditioning of the GLOBAL fit's LM steps (handles with S > 1 on a specialised kernel set).  The reference's driver
 * QR-factors the tall (m S) x q Jacobian (src/solvers/levmar/mod.rs:172-186 + qrfac via :247); the device step works on
 * J^T J accumulated over the right-hand sides and is exact to ~10 cond(J)^2 eps (measured within that
 * bound to cond(J) = 3.9e4).  cond_out[b] = the largest estimate of cond(J D^-1) -- J with normalised columns, as the LM
 * driver sees it -- over the steps of the last vp_fit (ratio of the extreme diagonal entries of the pivoted factor): a
 * caller who needs the QR-grade step beyond cond ~ 1e5 can tell from it that a fit ran there.  [B] doubles, host or
 * device pointer like every other array of the handle. */
int vp_global_fit_condition(vp_batch *h, double *cond_out);

/* same aggregates written to 4 DEVICE doubles, enqueued on the handle's stream without any host
 * synchronisation: the buffer can be handed straight to ncclAllReduce (RCCL) */
int vp_summary_device(vp_batch *h, double *dev_out4);

/*
 * The scalar LM cost reduction of SURVEY.md 8(b) / 8(e) for hosts WITHOUT a collective layer of their own (plain C / C++ /
 * Rust; Python callers use torch.distributed on vp_summary_device): the handle's aggregates
 * { sum 1/2||r||^2, #successful, #failed, sum n_evals } summed over all ranks of `rccl_comm` (an ncclComm_t) by ONE
 * ncclAllReduce of 4 doubles on the handle's stream -- 32 bytes over xGMI -- and returned in HOST doubles.  The library
 * does not link RCCL: ncclAllReduce is resolved at the first call from the process (a host that links librccl) or, failing
 * that, from librccl.so.1 (dlopen); VP_ERR_UNSUPPORTED if neither is there.  rccl_comm == NULL: the local aggregates
 * (== vp_summary).  Every rank of the communicator must make the call (it is a collective).
 */
int vp_reduce_cost(vp_batch *h, void *rccl_comm, double out[4]);

/*
 * One global fit whose right-hand sides are SHARDED over ranks (second row).  The reference fits
 * all S columns with one shared alpha (src/solvers/levmar/mod.rs:42-73, 154-186); here every rank owns a handle
 * with its block of the S columns (same model, grid, weights; B problems each) and vp_fit needs ONE exchange per
 * LM evaluation: the reduced sums {sum ||r||^2, sum c c^T, sum c_j G_p^T r} of the local columns, B*(1+n*n+p)
 * doubles.  The library leaves the collective to the caller: `fn` must sum `count` DEVICE doubles in place over
 * all ranks, ordered on `hip_stream` (ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, comm, hip_stream) on
 * RCCL), and return 0.  Every rank then runs the identical LM step on identical totals.
 *   global_rhs_count   S of the whole problem (the LM driver's residual count is m * global_rhs_count)
 *   fn == NULL         back to an unsharded handle
 * After vp_fit: alpha and the report (objective = global 1/2 sum ||r||^2) are identical on every rank; C, the
 * residual cache and vp_cost cover the local columns only.
 */
typedef int (*vp_allreduce_fn)(void *dev_doubles, int64_t count, void *hip_stream, void *user);
int vp_set_rhs_allreduce(vp_batch *h, vp_allreduce_fn fn, void *user, int64_t global_rhs_count);

/* Single-RHS fit kernel selection of a handle (explicit state; the library reads no environment variables).
 *   AUTO  : the persistent slot kernel (a wavefront owns several problems whose LM bookkeeping runs lane-parallel,
 *           problems are handed out from a device-side queue) once the batch exceeds the device's resident
 *           wavefront slots, otherwise one wavefront per problem; cases the slot kernel does not cover (weights,
 *           per-problem grids, models without a trailing constant basis) always run one wavefront per problem
 *   WAVE  : always one wavefront per problem
 *   SLOTS : the slot kernel whenever it covers the problem, regardless of the batch size
 * All three implement LevenbergMarquardt::minimize (src/solvers/levmar/mod.rs:247) with identical arithmetic per
 * problem; results do not depend on which wavefront or slot ran a problem.
 * VP_F32 handles whose model needs more than one wavefront's registers (five exponentials + offset beyond 128 rows,
 * BASELINE.json configs[4]) are fitted on the fp64 Gram matrix of [Phi | y | dPhi] (normal equations in double, any grid,
 * any weights) WHATEVER the selection: there is no fp32 Householder fit kernel for these shapes (it lost 15 % of the fits
 * to non-finite evaluations); vp_evaluate / vp_residuals / vp_jacobian / vp_statistics keep the fp32 Householder kernels. */
enum { VP_FIT_KERNEL_AUTO = 0, VP_FIT_KERNEL_WAVE = 1, VP_FIT_KERNEL_SLOTS = 2 };
int vp_set_fit_kernel(vp_batch *h, int which);

/* ---- introspection --------------------------------------------------------------------- */

/* duration in ms of the most recent launch of a kernel family on this handle, measured
 * with hipEvents on the handle's stream (enabled by vp_set_timing(h,1)). */
enum { VP_KERNEL_EVALUATE = 0, VP_KERNEL_BASIS = 1, VP_KERNEL_FIT = 2 };
int vp_set_timing(vp_batch *h, int enable);
int vp_last_kernel_ms(vp_batch *h, int which, float *ms);

int vp_synchronize(vp_batch *h);
const char *vp_last_error(void);
int vp_last_error_detail(void);
const char *vp_version(void);
/* number of visible HIP devices (0 if none); never fails */
int vp_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* VARPRO_HIP_H */
