"""Host-side mirror of the reference's model layer for the GPU path.

Reference: ``SeparableModelBuilder`` (src/model/builder/mod.rs:252-272, methods :338-525, validity
check :535-571), ``SeparableModel`` (src/model/mod.rs:367-517) and the plugin trait
``SeparableNonlinearModel`` (src/model/mod.rs:239-363).

The reference hands the solver opaque Rust closures; those cannot run on a GPU.  The
drop-in replaces "closure" by "basis kind" from a closed descriptor language (``basis.*``), keeping
the builder's call sequence, argument meaning and error variants: ``function(params, kind)`` /
``partial_deriv(param)`` / ``invariant_function(kind)`` / ``independent_variable(x)`` /
``initial_parameters(p)`` / ``build()``.  Derivatives are built into each kind; ``partial_deriv``
only declares (and validates) that the derivative is provided, exactly where the reference takes
the derivative closure.
"""
import numpy as np

from . import _lib


class basis:
    """basis-function kinds (include/varpro_hip.h): f(t, p0[, p1])"""
    CONST = 0       # 1                     (invariant_function)
    EXP_DECAY = 1   # exp(-t/p0)            shared_test_code/src/lib.rs:101-114
    EXP_RATE = 2    # exp(-p0 t)
    EXP_COS = 3     # exp(-p0 t) cos(p1 t)  shared_test_code/src/models.rs:310-372
    SIN_PHASE = 4   # sin(p0 t + p1)        src/test_helpers/mod.rs:28-52
    # (5 == VP_BASIS_EXTERNAL: a model the caller evaluates, ExternalModel below)
    GAUSS = 6       # exp(-(t - p0)^2 / (2 p1^2))     peak at p0, standard deviation p1
    LORENTZ = 7     # p1^2 / ((t - p0)^2 + p1^2)      peak at p0, half width at half maximum p1
    LINEAR = 8      # t                     (invariant_function: a sloped baseline)
    # IRF reconvolution on a UNIFORM grid of step dt, rho = exp(-dt/p0); irf: the instrument response of the problem
    # (BatchProblem(..., irf=) / set_irf, SeparableProblemBuilder.instrument_response).  Rectangle rule: lag 0 included, no dt
    EXP_DECAY_IRF = 9   # sum_{k<=i} irf_k rho^(i-k)      the decay exp(-t/p0) convolved with the response
    IRF = 10            # irf_i                 (invariant_function: the scattered-light term)
    # ... with the response repeating every period T >= m dt (BatchProblem(..., irf_period=) / set_irf_period; default: the
    # record is one period): the steady state of the pulse train, for decays that outlast the laser period
    EXP_DECAY_IRF_PERIODIC = 11  # sum_{p>=0} sum_k irf_k rho^(i-k+pP), P = T/dt   (terms with i-k+pP >= 0)
    # ... on the response SHIFTED by delta (grid units, positive: later; the last parameter of the function): kinds 9 - 11 on
    # g_i = r(i - delta/dt), r the Catmull-Rom cubic through the samples, zero outside the record (irf_shifted below).  All
    # shifted functions of a model name the SAME delta, and no other function may depend on it
    EXP_DECAY_IRF_SHIFT = 12           # kind 9 on g       (p0 = tau, p1 = delta)
    IRF_SHIFT = 13                     # g_i               (p0 = delta): the scattered-light term, shifted
    EXP_DECAY_IRF_PERIODIC_SHIFT = 14  # kind 11 on g      (p0 = tau, p1 = delta)
    ARITY = {CONST: 0, EXP_DECAY: 1, EXP_RATE: 1, EXP_COS: 2, SIN_PHASE: 2, GAUSS: 2, LORENTZ: 2, LINEAR: 0,
             EXP_DECAY_IRF: 1, IRF: 0, EXP_DECAY_IRF_PERIODIC: 1, EXP_DECAY_IRF_SHIFT: 2, IRF_SHIFT: 1,
             EXP_DECAY_IRF_PERIODIC_SHIFT: 2}
    NAME = {CONST: "const", EXP_DECAY: "exp_decay", EXP_RATE: "exp_rate", EXP_COS: "exp_cos", SIN_PHASE: "sin_phase",
            GAUSS: "gauss", LORENTZ: "lorentz", LINEAR: "linear", EXP_DECAY_IRF: "exp_decay_irf", IRF: "irf",
            EXP_DECAY_IRF_PERIODIC: "exp_decay_irf_periodic", EXP_DECAY_IRF_SHIFT: "exp_decay_irf_shift",
            IRF_SHIFT: "irf_shift", EXP_DECAY_IRF_PERIODIC_SHIFT: "exp_decay_irf_periodic_shift"}
    # kinds that read the response shifted, and those with a period
    SHIFT_KINDS = (EXP_DECAY_IRF_SHIFT, IRF_SHIFT, EXP_DECAY_IRF_PERIODIC_SHIFT)
    PERIODIC_KINDS = (EXP_DECAY_IRF_PERIODIC, EXP_DECAY_IRF_PERIODIC_SHIFT)
    # kinds that need the instrument response
    IRF_KINDS = (EXP_DECAY_IRF, IRF, EXP_DECAY_IRF_PERIODIC) + SHIFT_KINDS
    # kinds whose columns the device evaluates into memory (a device-column handle, include/varpro_hip.h)
    DEVICE_COLUMN = (GAUSS, LORENTZ, LINEAR, EXP_DECAY_IRF, IRF, EXP_DECAY_IRF_PERIODIC) + SHIFT_KINDS


def uniform_step(x, what="grid"):
    """dt = (x[-1] - x[0]) / (m - 1) of a grid the IRF kinds accept (last axis; m == 1: 0), ValueError where
    |x_i - x_0 - i dt| > 1e-6 |dt| (include/varpro_hip.h, "IRF reconvolution")"""
    x = np.asarray(x, dtype=np.float64)
    m = x.shape[-1]
    if m == 1:
        return np.zeros(x.shape[:-1])
    dt = (x[..., -1] - x[..., 0]) / (m - 1)
    dev = np.abs(x - x[..., :1] - np.arange(m) * dt[..., None])
    if not np.all(dev <= 1e-6 * np.abs(dt)[..., None]):
        raise ValueError("NonUniformGrid: the IRF reconvolution kinds need a uniform %s: |x_i - x_0 - i dt| <= 1e-6 |dt|" % what)
    return dt


def check_irf(irf, B, m):
    """(irf, per_problem) for a batch of B problems of m samples: shape (m,) shared or (B, m); ValueError otherwise"""
    shape = tuple(int(s) for s in irf.shape)
    if shape == (m,):
        return irf, False
    if shape == (B, m):
        return irf, True
    raise ValueError("InvalidLengthOfIrf: the instrument response must have shape (%d,) or (%d, %d), got %r" % (m, B, m, shape))


def check_irf_period(period, m=None, dt=None):
    """the period of basis.EXP_DECAY_IRF_PERIODIC as a float (None / 0: the record is one period); ValueError for NaN, a
    negative value and, given the steps dt of host grids of m samples, period < m dt (1 - 1e-6) on any of them"""
    period = 0.0 if period is None else float(period)
    if not period >= 0:
        raise ValueError("InvalidIrfPeriod: the period must be 0 (the record is one period) or positive, got %r" % (period,))
    if period > 0 and dt is not None and np.any(period < m * np.asarray(dt, dtype=np.float64) * (1 - 1e-6)):
        raise ValueError("InvalidIrfPeriod: the period %r is shorter than the record, m dt = %r"
                         % (period, float(np.max(m * np.asarray(dt, dtype=np.float64)))))
    return period


def irf_columns(irf, dt, tau, period=None):
    """numpy mirror of the scan kernel (vp_irf.hpp), the plain sequential recurrence in the dtype of irf:
    F_i = irf_i + rho F_{i-1}, H_i = rho (H_{i-1} + F_{i-1}), rho = exp(-dt/tau) -> (F, dt/tau^2 H).
    period: None -- F_{-1} = H_{-1} = 0 (basis.EXP_DECAY_IRF); else the periodic form (basis.EXP_DECAY_IRF_PERIODIC) with
    T = period, 0: T = m dt.  A totals pass gives A = F_{m-1}, B = H_{m-1} of the zero start, then the same recurrence runs
    from the steady-state carry (include/varpro_hip.h): with g = (T - m dt)/dt, P = m + g, e = exp(-(T - m dt)/tau),
    E = exp(-T/tau), D = -expm1(-T/tau):  F_{-1} = e A / D,  H_{-1} = (e/D) (g A + B + P E A / D).
    T < m dt (1 - 1e-6) gives NaN columns, inside that band g = 0."""
    irf = np.asarray(irf)
    T = irf.dtype.type
    dt, tau = T(dt), T(tau)
    m = irf.size
    F, H = np.empty_like(irf), np.empty_like(irf)
    with np.errstate(all="ignore"):
        span = T(m) * dt
        gap = T(0)
        if period is not None and T(period) > 0:
            gap = T(period) - span
            if gap < T(-1e-6) * span:
                tau = T(np.nan)
            if not gap > 0:
                gap = T(0)
        rho = np.exp(-(dt / tau)) if tau > 0 else T(np.nan)
        f = h = T(0)
        v = irf
        if irf.dtype == np.float64:  # (Python floats are IEEE doubles: the same roundings, a faster loop)
            rho, f, h, v = float(rho), 0.0, 0.0, irf.tolist()
        if period is not None:
            for i in range(m):  # the totals of the zero start at row m - 1
                h = rho * (h + f)
                f = v[i] + rho * f
            f, h = T(f), T(h)
            per = span + gap
            g = gap / dt
            e = np.exp(-(gap / tau)) if gap > 0 else T(1)
            E, D = np.exp(-(per / tau)), -np.expm1(-(per / tau))
            f, h = (e * f) / D, (e / D) * (g * f + h + (T(m) + g) * E * f / D)
            if irf.dtype == np.float64:
                f, h = float(f), float(h)
        for i in range(m):
            h = rho * (h + f)
            f = v[i] + rho * f
            F[i], H[i] = f, h
        return F, (dt / (tau * tau)) * H


def irf_shifted(irf, dt, delta):
    """numpy mirror of the resample kernel (vp_irf_shift.hpp) in the dtype of irf: (g, g') with g_i = r(i - s), s = delta/dt,
    r the Catmull-Rom cubic through the samples and zero outside the record, g' = dg/ddelta (include/varpro_hip.h,
    "Shifted IRF reconvolution"):  o = floor(-s), f = -s - o,  g_i = sum_{a=-1..2} w_a(f) irf_{i+o+a},
    g'_i = -(1/dt) sum_a w'_a(f) irf_{i+o+a}.  A non-finite s gives NaN, |s| >= m + 2 exact zeros, delta = 0 the response."""
    irf = np.asarray(irf)
    T = irf.dtype.type
    m = irf.size
    with np.errstate(all="ignore"):
        dt = T(dt)
        ns = -(T(delta) / dt)
        if not abs(ns) < T(m + 2):
            v = T(0) if np.isfinite(ns) else T(np.nan)
            return np.full(m, v, irf.dtype), np.full(m, v, irf.dtype)
        fl = np.floor(ns)
        o, f = int(fl), T(ns - fl)
        h, ff = T(0.5), f * f
        w = (h * (f * ((T(2) - f) * f - T(1))), h * (ff * (T(3) * f - T(5)) + T(2)),
             h * (f * ((T(4) - T(3) * f) * f + T(1))), h * (ff * (f - T(1))))
        d = (h * ((T(4) - T(3) * f) * f - T(1)), h * (f * (T(9) * f - T(10))),
             h * ((T(8) - T(9) * f) * f + T(1)), h * (f * (T(3) * f - T(2))))
        pad = np.zeros(3 * m + 8, irf.dtype)  # irf_k at pad[k + m + 4]: every tap of |o| <= m + 2 is inside
        pad[m + 4:2 * m + 4] = irf
        taps = [pad[m + 4 + o + a:2 * m + 4 + o + a] for a in (-1, 0, 1, 2)]
        g = ((w[0] * taps[0] + w[1] * taps[1]) + w[2] * taps[2]) + w[3] * taps[3]
        dg = -(((d[0] * taps[0] + d[1] * taps[1]) + d[2] * taps[2]) + d[3] * taps[3]) / dt
        return g.astype(irf.dtype), dg.astype(irf.dtype)


def _kind_columns(kind, x, p0, p1, irf=None, irf_period=None):
    """numpy mirror of one basis kind: (f, [df/dp0, df/dp1][:arity]) on the grid x (include/varpro_hip.h)"""
    if kind in basis.IRF_KINDS:
        if irf is None:
            raise ModelError("the model has an IRF reconvolution kind and no instrument response (model.irf)")
        if kind in basis.SHIFT_KINDS:  # the unshifted kind on g; d/ddelta: its value column on g'
            dt = uniform_step(x)
            g, dg = irf_shifted(np.asarray(irf, dtype=x.dtype), dt, p0 if kind == basis.IRF_SHIFT else p1)
            if kind == basis.IRF_SHIFT:
                return g, [dg]
            period = (irf_period or 0.0) if kind == basis.EXP_DECAY_IRF_PERIODIC_SHIFT else None
            f, dtau = irf_columns(g, dt, p0, period)
            return f, [dtau, irf_columns(dg, dt, p0, period)[0]]
        if kind == basis.IRF:
            return np.array(irf, dtype=x.dtype), []
        period = (irf_period or 0.0) if kind == basis.EXP_DECAY_IRF_PERIODIC else None
        f, d = irf_columns(np.asarray(irf, dtype=x.dtype), uniform_step(x), p0, period)
        return f, [d]
    if kind == basis.CONST:
        return np.ones_like(x), []
    if kind == basis.LINEAR:
        return x.copy(), []
    if kind == basis.EXP_DECAY:
        f = np.exp(-x / p0)
        return f, [f * x / p0 ** 2]
    if kind == basis.EXP_RATE:
        f = np.exp(-p0 * x)
        return f, [-x * f]
    if kind == basis.EXP_COS:
        e = np.exp(-p0 * x)
        f = e * np.cos(p1 * x)
        return f, [-x * f, -x * e * np.sin(p1 * x)]
    if kind == basis.SIN_PHASE:
        c = np.cos(p0 * x + p1)
        return np.sin(p0 * x + p1), [x * c, c]
    if kind == basis.GAUSS:
        f = np.exp(-0.5 * ((x - p0) / p1) ** 2)
        return f, [f * (x - p0) / p1 ** 2, f * (x - p0) ** 2 / p1 ** 3]
    if kind == basis.LORENTZ:
        den = (x - p0) ** 2 + p1 ** 2
        return p1 ** 2 / den, [2 * p1 ** 2 * (x - p0) / den ** 2, 2 * p1 * (x - p0) ** 2 / den ** 2]
    raise ModelError("unknown basis kind %r" % (kind,))


class ModelBuildError(ValueError):
    """mirrors varpro::model::builder::error::ModelBuildError (src/model/builder/error.rs)"""

    def __init__(self, variant, message):
        super().__init__("%s: %s" % (variant, message))
        self.variant = variant


class ModelError(RuntimeError):
    """mirrors varpro::model::errors::ModelError (derivative index out of bounds etc.)"""


class SeparableModel:
    """A separable model  f(x, alpha, c) = sum_j c_j phi_j(x, alpha)  described by basis kinds.

    Implements the ``SeparableNonlinearModel`` surface: ``parameter_count``, ``base_function_count``,
    ``output_len``, ``set_params``, ``params``, ``eval``, ``eval_partial_deriv`` (the last two run
    the stand-alone Phi kernel, ``vp_basis``).
    """

    def __init__(self, parameter_names, kinds, params, x, initial_parameters, dtype=np.float64):
        self.parameter_names = list(parameter_names)
        self.kinds = [int(k) for k in kinds]
        self.param_indices = [tuple(int(i) for i in p) for p in params]
        self.n_params = len(self.parameter_names)
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise TypeError("ScalarType must be float64 or float32")
        self.x = np.ascontiguousarray(x, dtype=self.dtype).reshape(-1)
        self._alpha = np.ascontiguousarray(initial_parameters, dtype=self.dtype).reshape(-1)
        self.irf = None  # IRF kinds: the response of the single-problem surface (SeparableProblemBuilder.instrument_response)
        self.irf_period = None  # ... and the period of basis.EXP_DECAY_IRF_PERIODIC (None / 0: the record is one period)
        # dependency pairs in model order (basis-major): the layout of vp_basis' dPhi output
        self.pairs = [(j, a, pi) for j, ps in enumerate(self.param_indices) for a, pi in enumerate(ps)]

    # -- SeparableNonlinearModel surface (src/model/mod.rs:256-271) --
    def parameter_count(self):
        return self.n_params

    def base_function_count(self):
        return len(self.kinds)

    def output_len(self):
        return int(self.x.size)

    def set_params(self, parameters):
        p = np.ascontiguousarray(parameters, dtype=self.dtype).reshape(-1)
        if p.size != self.n_params:
            raise ModelError("IncorrectParameterCount: expected %d, got %d" % (self.n_params, p.size))
        self._alpha = p.copy()

    def params(self):
        return self._alpha.copy()

    def desc(self):
        d = _lib.ModelDesc()
        d.n_basis = len(self.kinds)
        d.n_params = self.n_params
        for j in range(_lib.VP_MAX_BASIS):
            d.kind[j] = 0
            for a in range(_lib.VP_MAX_BASIS_PARAMS):
                d.param[j][a] = -1
        for j, (k, ps) in enumerate(zip(self.kinds, self.param_indices)):
            d.kind[j] = k
            for a, pi in enumerate(ps):
                d.param[j][a] = pi
        return d

    def _basis_host(self):
        """Phi (1, n, m), dPhi (1, p, m) in numpy: the host mirror of the column kernel (vp_cols.hpp)"""
        x = self.x
        a = self._alpha
        phi = np.empty((1, len(self.kinds), x.size), dtype=self.dtype)
        dphi = np.empty((1, len(self.pairs), x.size), dtype=self.dtype)
        pair = 0
        with np.errstate(all="ignore"):
            for j, (kind, ps) in enumerate(zip(self.kinds, self.param_indices)):
                args = [a[pi] for pi in ps] + [None, None]
                f, ds = _kind_columns(kind, x, args[0], args[1], self.irf, self.irf_period)
                phi[0, j] = f
                for d in ds:
                    dphi[0, pair] = d
                    pair += 1
        return phi, dphi

    def _basis(self):
        # peak / baseline kinds: the model surface is evaluated on the host (the device evaluates them for BatchProblem)
        if any(k in basis.DEVICE_COLUMN for k in self.kinds):
            return self._basis_host()
        from .batch import BatchProblem
        # a data-free handle is enough for the Phi kernel; y is a dummy column
        bp = BatchProblem(self, np.zeros((1, self.x.size), dtype=self.dtype), x=self.x)
        return bp.basis(self._alpha.reshape(1, -1))

    def eval(self):
        """Phi(alpha): (m, n) matrix, column j = basis j  (src/model/mod.rs:308)"""
        phi, _ = self._basis()
        return np.ascontiguousarray(phi[0].T)

    def eval_partial_deriv(self, derivative_index):
        """dPhi/dalpha_k: (m, n), zero columns for independent basis functions (src/model/mod.rs:359-362)"""
        k = int(derivative_index)
        if k < 0 or k >= self.n_params:
            raise ModelError("DerivativeIndexOutOfBounds: %d" % k)
        _, dphi = self._basis()
        out = np.zeros((self.x.size, len(self.kinds)), dtype=self.dtype)
        for p, (j, _a, pi) in enumerate(self.pairs):
            if pi == k:
                out[:, j] += dphi[0, p]
        return out


class ExternalModel:
    """Shape of a model the CALLER evaluates: any ``SeparableNonlinearModel`` (src/model/mod.rs:239-363), e.g. the
    reference's closure-based ``SeparableModel`` (src/model/mod.rs:441-512), whose basis functions the closed descriptor
    language above cannot express.  Only what the device needs: n basis functions, q parameters and the
    (basis j, parameter k) pairs with a non-zero derivative -- the columns ``eval_partial_deriv(k)`` fills
    (src/model/mod.rs:473-512).  ``BatchProblem(ExternalModel(...), Y)`` makes a handle with
    ``vp_batch_create_external``; Phi / dPhi then enter through ``set_params_with_basis`` /
    ``jacobian_with_derivatives`` / ``evaluate_with_basis``.  ``ClosureModel`` builds one from Python callables."""

    def __init__(self, n_basis, n_params, pairs, dtype=np.float64):
        self.n_basis, self.n_params = int(n_basis), int(n_params)
        self.ext_pairs = [(int(j), int(k)) for j, k in pairs]
        self.pairs = self.ext_pairs  # len() == number of derivative columns
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise TypeError("ScalarType must be float64 or float32")
        self.x = None

    def parameter_count(self):
        return self.n_params

    def base_function_count(self):
        return self.n_basis


class ClosureModel:
    """== the reference's closure-based ``SeparableModel`` (src/model/mod.rs:367-517, built by
    ``SeparableModelBuilder::function(params, f).partial_deriv(param, df)``, src/model/builder/mod.rs:338-525) with REAL
    Python callables: ``f(x, *params) -> (m,)`` evaluated on the host with numpy for a whole batch of parameter sets.
    ``eval_batch(alpha (B, q)) -> Phi (B, n, m)`` and ``derivs_batch(alpha) -> dPhi (B, p, m)`` produce exactly what
    ``BatchProblem.set_params_with_basis`` takes; ``shape()`` is the matching ``ExternalModel``."""

    def __init__(self, parameter_names, x, dtype=np.float64):
        self.names = list(parameter_names)
        # the builder's checks on the model parameter list (src/model/builder/mod.rs:338-370, error.rs variant names)
        if len(self.names) == 0:
            raise ModelBuildError("EmptyParameters", "A function or model parameter list is empty!")
        if len(set(self.names)) != len(self.names):
            raise ModelBuildError("DuplicateParameterNames", "Parameter list %r contains duplicates!" % (self.names,))
        if any("," in n for n in self.names):
            raise ModelBuildError("CommaInParameterNameNotAllowed", "Parameter names may not contain comma separator")
        self.x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        self.dtype = np.dtype(dtype)
        self._functions = []  # (param indices, f, {param index: df})

    def invariant_function(self, f):
        self._functions.append(((), f, {}))
        return self

    def function(self, function_params, f):
        fp = list(function_params)
        if len(fp) == 0:
            raise ModelBuildError("EmptyParameters", "A function or model parameter list is empty!")
        if len(set(fp)) != len(fp):
            raise ModelBuildError("DuplicateParameterNames", "Parameter list %r contains duplicates!" % (fp,))
        for p in fp:
            if p not in self.names:
                raise ModelBuildError("FunctionParameterNotInModel",
                                      "Function parameter '%s' is not part of the model parameters." % p)
        idx = tuple(self.names.index(p) for p in fp)
        self._functions.append((idx, f, {}))
        return self

    def partial_deriv(self, parameter, df):
        if not self._functions or not self._functions[-1][0]:
            # (the reference's builder has no partial_deriv in the state that follows an invariant function: a type error there)
            raise ModelBuildError("InvalidDerivative", "partial_deriv needs a preceding function with parameters")
        idx, _f, derivs = self._functions[-1]
        if parameter not in self.names:
            raise ModelBuildError("InvalidDerivative", "Parameter '%s' is not in the function's parameter list" % parameter)
        k = self.names.index(parameter)
        if k not in idx:
            raise ModelBuildError("InvalidDerivative", "Parameter '%s' is not in the function's parameter list" % parameter)
        if k in derivs:
            raise ModelBuildError("DuplicateDerivative", "Derivative for parameter '%s' was already provided!" % parameter)
        derivs[k] = df
        return self

    def pairs(self):
        return [(j, k) for j, (idx, _f, _d) in enumerate(self._functions) for k in idx]

    def shape(self):
        # == SeparableModelBuilder::build (src/model/builder/mod.rs:527-553): EmptyModel, MissingDerivative, UnusedParameter
        if not self._functions:
            raise ModelBuildError("EmptyModel", "A model must contain at least one function")
        for idx, _f, derivs in self._functions:
            for k in idx:
                if k not in derivs:
                    raise ModelBuildError("MissingDerivative", "missing derivative for parameter '%s'" % self.names[k])
        used = {k for idx, _f, _d in self._functions for k in idx}
        for k, name in enumerate(self.names):
            if k not in used:
                raise ModelBuildError("UnusedParameter", "Parameter '%s' is not used by any function of the model" % name)
        return ExternalModel(len(self._functions), len(self.names), self.pairs(), dtype=self.dtype)

    def eval_batch(self, alpha):
        """== eval() (src/model/mod.rs:441-471) for every parameter set of the batch: (B, n, m), UNWEIGHTED"""
        a = np.asarray(alpha, dtype=np.float64).reshape(-1, len(self.names))
        out = np.empty((a.shape[0], len(self._functions), self.x.size), dtype=self.dtype)
        for b in range(a.shape[0]):
            for j, (idx, f, _d) in enumerate(self._functions):
                out[b, j] = f(self.x, *[a[b, k] for k in idx])
        return out

    def derivs_batch(self, alpha):
        """== the non-zero columns of eval_partial_deriv(k) (src/model/mod.rs:473-512) in pair order: (B, p, m)"""
        a = np.asarray(alpha, dtype=np.float64).reshape(-1, len(self.names))
        prs = self.pairs()
        out = np.empty((a.shape[0], len(prs), self.x.size), dtype=self.dtype)
        for b in range(a.shape[0]):
            for p, (j, k) in enumerate(prs):
                idx, _f, derivs = self._functions[j]
                out[b, p] = derivs[k](self.x, *[a[b, kk] for kk in idx])
        return out


class SeparableModelBuilder:
    """mirrors ``SeparableModelBuilder`` (src/model/builder/mod.rs:338-525)"""

    def __init__(self, parameter_names, dtype=np.float64):
        self._error = None
        self._names = list(parameter_names)
        self._dtype = dtype
        self._functions = []  # dicts: params(list of names), kind, derivs(set)
        self._x = None
        self._initial = None
        self._building = False  # state FunctionBuilding
        if len(self._names) == 0:
            self._fail("EmptyParameters", "A function or model parameter list is empty!")
        elif len(set(self._names)) != len(self._names):
            self._fail("DuplicateParameterNames", "Parameter list %r contains duplicates!" % (self._names,))
        elif any("," in n for n in self._names):
            self._fail("CommaInParameterNameNotAllowed", "Parameter names may not contain comma separator")

    @classmethod
    def new(cls, parameter_names, dtype=np.float64):
        return cls(parameter_names, dtype)

    def _fail(self, variant, msg):
        if self._error is None:
            self._error = ModelBuildError(variant, msg)
        return self

    def invariant_function(self, kind=basis.CONST):
        if self._error:
            return self
        if basis.ARITY.get(kind) != 0:
            return self._fail("IncorrectParameterCount", "invariant function takes no parameters")
        self._functions.append(dict(params=[], kind=kind, derivs=set()))
        self._building = False
        return self

    def function(self, function_params, kind):
        if self._error:
            return self
        fp = list(function_params)
        if len(fp) == 0:
            return self._fail("EmptyParameters", "A function or model parameter list is empty!")
        if len(set(fp)) != len(fp):
            return self._fail("DuplicateParameterNames", "Parameter list %r contains duplicates!" % (fp,))
        for p in fp:
            if p not in self._names:
                return self._fail("FunctionParameterNotInModel",
                                  "Function parameter '%s' is not part of the model parameters." % p)
        if kind not in basis.ARITY:
            return self._fail("IncorrectParameterCount", "unknown basis kind %r" % (kind,))
        if basis.ARITY[kind] != len(fp):
            return self._fail("IncorrectParameterCount", "Incorrect number of parameters for function: expected %d, "
                              "got %d" % (basis.ARITY[kind], len(fp)))
        self._functions.append(dict(params=fp, kind=kind, derivs=set()))
        self._building = True
        return self

    def partial_deriv(self, parameter, _derivative=None):
        if self._error:
            return self
        if not self._building:
            return self._fail("IllegalCallToPartialDeriv", "a call to this function can only follow a call to "
                              "'function' or another call to 'partial_deriv'")
        f = self._functions[-1]
        if parameter not in f["params"]:
            return self._fail("InvalidDerivative", "Parameter '%s' given for partial derivative does not exist in "
                              "parameter list '%r'." % (parameter, f["params"]))
        if parameter in f["derivs"]:
            return self._fail("DuplicateDerivative", "Derivative for parameter '%s' was already provided!" % parameter)
        f["derivs"].add(parameter)
        return self

    def independent_variable(self, x):
        if self._error:
            return self
        self._x = np.asarray(x)
        self._building = False
        return self

    def initial_parameters(self, initial):
        if self._error:
            return self
        init = np.asarray(initial, dtype=np.float64).reshape(-1)
        if init.size != len(self._names):
            return self._fail("IncorrectParameterCount", "Incorrect number of parameters for function: expected %d, "
                              "got %d" % (len(self._names), init.size))
        self._initial = init
        self._building = False
        return self

    def build(self):
        if self._error:
            raise self._error
        if not self._functions:
            raise ModelBuildError("EmptyModel", "Tried to construct model with no functions.")
        for f in self._functions:
            for p in f["params"]:
                if p not in f["derivs"]:
                    raise ModelBuildError("MissingDerivative", "Function with paramter list %r is missing derivative "
                                          "for parametr '%s'." % (f["params"], p))
        used = set(p for f in self._functions for p in f["params"])
        for n in self._names:
            if n not in used:
                raise ModelBuildError("UnusedParameter", "Model depends on parameter '%s', but none of its functions "
                                      "use it." % n)
        # one response, one shift: every shifted function names the same delta, nothing else depends on it
        deltas = [(f["params"][-1], f["kind"]) for f in self._functions if f["kind"] in basis.SHIFT_KINDS]
        if deltas:
            for name, kind in deltas:
                if name != deltas[0][0]:
                    raise ModelBuildError("SeveralIrfShifts", "the functions of kind %s and %s name different shift parameters "
                                          "'%s' and '%s': a model has one response and one shift"
                                          % (basis.NAME[deltas[0][1]], basis.NAME[kind], deltas[0][0], name))
            for f in self._functions:
                others = f["params"][:-1] if f["kind"] in basis.SHIFT_KINDS else f["params"]
                if deltas[0][0] in others:
                    raise ModelBuildError("IrfShiftShared", "the shift parameter '%s' of kind %s is also a parameter of a function "
                                          "of kind %s: no other function may depend on it"
                                          % (deltas[0][0], basis.NAME[deltas[0][1]], basis.NAME[f["kind"]]))
        if self._x is None:
            raise ModelBuildError("MissingX", "Missing vector for independent variable x")
        if any(f["kind"] in basis.IRF_KINDS for f in self._functions):
            try:
                uniform_step(np.asarray(self._x).reshape(-1), "independent variable")
            except ValueError as e:
                raise ModelBuildError("NonUniformGrid", str(e))
        if self._initial is None:
            raise ModelBuildError("MissingInitialParameters", "Missing initial guesses for model parameters")
        if len(self._functions) > _lib.VP_MAX_BASIS or len(self._names) > _lib.VP_MAX_PARAMS:
            raise ModelBuildError("IncorrectParameterCount", "model exceeds VP_MAX_BASIS/VP_MAX_PARAMS")
        kinds = [f["kind"] for f in self._functions]
        params = [tuple(self._names.index(p) for p in f["params"]) for f in self._functions]
        return SeparableModel(self._names, kinds, params, self._x, self._initial, dtype=self._dtype)


def multi_exponential_model(x, initial_taus, offset=True, dtype=np.float64):
    """sum of exponential decays exp(-x/tau_j) (+ constant): the model family of every bench in the
    reference (shared_test_code/src/lib.rs:119-135, shared_test_code/src/models.rs:16-156)."""
    taus = list(np.asarray(initial_taus, dtype=np.float64).reshape(-1))
    names = ["tau%d" % (i + 1) for i in range(len(taus))]
    b = SeparableModelBuilder(names, dtype=dtype)
    for nme in names:
        b = b.function([nme], basis.EXP_DECAY).partial_deriv(nme)
    if offset:
        b = b.invariant_function(basis.CONST)
    return b.independent_variable(x).initial_parameters(taus).build()
