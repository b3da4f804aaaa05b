"""BatchProblem: B independent separable problems (or B problems x S right-hand sides) on one GPU.

This is the Python face of the ``vp_batch`` handle (include/varpro_hip.h).  It holds what the
reference's ``SeparableProblem`` + ``CachedCalculations`` hold (src/problem.rs:57-107) for a whole
batch, resident in HBM, and exposes the ``LeastSquaresProblem`` surface
(src/solvers/levmar/mod.rs:22-202) batch-wise.

Array conventions (row index fastest, i.e. each problem's slice is the reference's column-major
matrix):  Y, R: (B, S, m) or (B, m) when S == 1;  alpha: (B, q);  C: (B, S, n) / (B, n);
J: (B, q, S, m) / (B, q, m).

Inputs may be numpy arrays (host-pointer mode: the library stages through HBM) or torch CUDA
tensors (device-pointer mode: zero copies, results are torch tensors on the same device and the
work is enqueued on torch's current stream).
"""
import ctypes as C

import numpy as np

from . import _lib, bounds as _bounds
from .model import basis as _basis, check_irf as _check_irf, check_irf_period as _check_irf_period, uniform_step as _uniform_step
from ._lib import check

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

REPORT_DTYPE = np.dtype([("termination", np.int32), ("n_evals", np.int32), ("objective", np.float64)])

STATUS_OK, STATUS_NONFINITE, STATUS_NOT_EVALUATED = 0, 1, 2

# fit_poisson: model-weighted rounds after the Neyman fit (measured on the CPU mirror)
POISSON_ROUNDS = 9
# fit_robust: re-weighted rounds after the fit at the base weights (measured on the CPU mirror)
ROBUST_ROUNDS = 14
ROBUST_LOSSES = {"huber": _lib.VP_ROBUST_HUBER, "cauchy": _lib.VP_ROBUST_CAUCHY, "tukey": _lib.VP_ROBUST_TUKEY}


def _is_torch(a):
    return torch is not None and isinstance(a, torch.Tensor)


class LevenbergMarquardt:
    """mirrors ``levenberg_marquardt::LevenbergMarquardt`` builder knobs (reached in the reference via
    ``LevMarSolver::with_solver``, src/solvers/levmar/mod.rs:221-223)."""

    def __init__(self, dtype=np.float64):
        eps = float(np.finfo(dtype).eps)
        self.ftol = self.xtol = self.gtol = 30.0 * eps
        self.stepbound = 100.0
        self.patience = 100
        self.scale_diag = True

    @classmethod
    def new(cls, dtype=np.float64):
        return cls(dtype)

    def with_ftol(self, v):
        self.ftol = float(v)
        return self

    def with_xtol(self, v):
        self.xtol = float(v)
        return self

    def with_gtol(self, v):
        self.gtol = float(v)
        return self

    def with_tol(self, v):
        self.ftol = self.xtol = self.gtol = float(v)
        return self

    def with_stepbound(self, v):
        self.stepbound = float(v)
        return self

    def with_patience(self, v):
        self.patience = int(v)
        return self

    def with_scale_diag(self, v):
        self.scale_diag = bool(v)
        return self

    def _c(self):
        o = _lib.LmOpts()
        o.ftol, o.xtol, o.gtol, o.stepbound = self.ftol, self.xtol, self.gtol, self.stepbound
        o.patience, o.scale_diag = self.patience, int(self.scale_diag)
        return o


def _to_host(a):
    return a.detach().cpu().numpy() if _is_torch(a) else a


def _tensors_in(obj):
    if _is_torch(obj):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _tensors_in(v)
    elif isinstance(obj, (tuple, list)):
        for v in obj:
            yield from _tensors_in(v)


def _device_entry(fn):
    """Stream discipline of device-pointer mode.  A handle enqueues all its work on ONE HIP stream: the stream that
    was current when the handle was created (one handle <-> one stream, include/varpro_hip.h).  If the caller's current
    stream is a different one, the call is bracketed: the handle's stream waits for the caller's stream (inputs
    ready), the body runs with the handle's stream current (so torch allocates the outputs there), the caller's stream
    waits for the handle's stream (outputs ready), and every tensor that crosses is recorded on the other stream so
    that the caching allocator does not recycle its memory while that stream still uses it."""
    import functools

    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        if not self.device_mode:
            return fn(self, *args, **kwargs)
        cur = torch.cuda.current_stream(self._tdev)
        hs = self._tstream
        if cur.cuda_stream == hs.cuda_stream:
            return fn(self, *args, **kwargs)
        hs.wait_stream(cur)
        for t in _tensors_in((args, kwargs)):
            if t.is_cuda:
                t.record_stream(hs)
        with torch.cuda.stream(hs):
            out = fn(self, *args, **kwargs)
        cur.wait_stream(hs)
        for t in _tensors_in(out):
            if t.is_cuda:
                t.record_stream(cur)
        return out

    return wrapper


class BatchProblem:
    def __new__(cls, *args, **kwargs):
        # fixed={...}: the subclass of varpro_amd/fixed.py keeps the books between the model's full parameter order and the
        # handle's reduced one; without it nothing below takes another path
        if cls is BatchProblem and kwargs.get("fixed") is not None:
            from .fixed import FixedBatchProblem
            return object.__new__(FixedBatchProblem)
        return object.__new__(cls)

    def __init__(self, model, Y, x=None, weights=None, epsilon=None, device=0, grid_recurrence=True, stream_rows=False,
                 device_columns=False, irf=None, irf_period=None, *, fixed=None):
        """model: varpro_amd.SeparableModel; Y: (B, m) or (B, S, m); x: (m,) shared grid or (B, m)
        per-problem grids (default: model.x); weights: None (unit), (m,) or (B, m).
        irf: the instrument response of a model with ``basis.EXP_DECAY_IRF`` / ``basis.IRF``, (m,) shared or (B, m)
        (``set_irf`` sets or replaces it later); such a model needs a uniform grid.
        irf_period: the period T >= m dt of ``basis.EXP_DECAY_IRF_PERIODIC`` in the units of the grid (``set_irf_period``);
        None or 0: the record is exactly one period.
        grid_recurrence=False sets VP_FLAG_NO_GRID_RECURRENCE (per-row exponentials even on uniform grids).
        device_columns=True sets VP_FLAG_DEVICE_COLUMNS: a descriptor of the exponential / trigonometric kinds alone becomes a
        device-column handle too, which takes ``set_bounds``.
        fixed: dict parameter name -> value (a scalar, or a (B,) array / tensor: one value per problem) of nonlinear
        parameters that are known and not fitted (vp_batch_create_fixed); the object is then a
        ``varpro_amd.fixed.FixedBatchProblem``, whose docstring says what takes and returns the full parameter order."""
        self.lib = _lib.load()
        self.model = model
        self.n = model.base_function_count()
        self.q = model.parameter_count()
        self.p = len(model.pairs)
        self.device_mode = _is_torch(Y)
        if self.device_mode:
            self._tdev = Y.device
        self.np_dtype = np.dtype(model.dtype)
        self.vp_dtype = _lib.VP_F64 if self.np_dtype == np.float64 else _lib.VP_F32
        self.external = hasattr(model, "ext_pairs")  # model.ExternalModel: the caller evaluates Phi / dPhi
        if fixed is not None and self.external:
            raise ValueError("fixed: a caller-evaluated model fixes its parameters in its own evaluation")
        if fixed is not None and not hasattr(self, "_create_handle"):
            raise ValueError("fixed: construct varpro_amd.BatchProblem itself, or derive from varpro_amd.fixed.FixedBatchProblem "
                             "(a subclass of BatchProblem has none of its full-order bookkeeping)")
        x = model.x if x is None else x
        Y = self._as_array(Y)
        if Y.ndim == 2:
            self.single_rhs = True
            B, m = Y.shape
            S = 1
        elif Y.ndim == 3:
            self.single_rhs = False
            B, S, m = Y.shape
        else:
            raise ValueError("Y must be (B, m) or (B, S, m)")
        self.B, self.S, self.m = int(B), int(S), int(m)
        if self.external:
            x = None
        else:
            x = self._as_array(x)
        flags = 0 if grid_recurrence else _lib.VP_FLAG_NO_GRID_RECURRENCE
        if stream_rows:  # VP_FLAG_STREAM_ROWS: the length-agnostic fit kernels even where a resident set covers m
            flags |= _lib.VP_FLAG_STREAM_ROWS
        if device_columns:
            flags |= _lib.VP_FLAG_DEVICE_COLUMNS
        if self.device_mode:
            flags |= _lib.VP_FLAG_DEVICE_PTRS  # work is enqueued on torch's current stream
        else:
            flags |= _lib.VP_FLAG_OWN_STREAM
        if x is None:
            pass  # a caller-evaluated model has no grid
        elif x.ndim == 2:
            flags |= _lib.VP_FLAG_T_PER_PROBLEM
            if tuple(x.shape) != (self.B, self.m):
                raise ValueError("per-problem grid must be (B, m)")
        elif int(x.shape[0]) != self.m:
            # SeparableProblemBuilderError::InvalidLengthOfData (src/problem/builder.rs:294-299)
            raise ValueError("InvalidLengthOfData: x length = %d and y length = %d" % (int(x.shape[0]), self.m))
        w = None
        if isinstance(weights, str):
            # Neyman weights of Poisson counts, w = 1/sqrt(max(y, 1)) per problem, formed where the data lives
            # ("unit": per-problem unit weights, the base of a robust fit of homoscedastic data)
            if weights not in ("neyman", "unit"):
                raise ValueError("weights: an array, None, \"neyman\" or \"unit\"")
            if not self.single_rhs:
                raise ValueError("weights=\"%s\": weights are per problem, not per right-hand side (S = 1 only)" % weights)
            if weights == "unit":
                weights = torch.ones_like(Y) if self.device_mode else np.ones_like(Y)
            else:
                one = Y.new_ones(()) if self.device_mode else self.np_dtype.type(1)
                weights = 1.0 / (torch.sqrt(torch.maximum(Y, one)) if self.device_mode else np.sqrt(np.maximum(Y, one)))
        if weights is not None:
            w = self._as_array(weights)
            if w.ndim == 2:
                flags |= _lib.VP_FLAG_W_PER_PROBLEM
                if tuple(w.shape) != (self.B, self.m):
                    raise ValueError("InvalidLengthOfWeights")
            elif int(w.shape[0]) != self.m:
                raise ValueError("InvalidLengthOfWeights")  # src/problem/builder.rs:300-303
        self.weighted = w is not None                     # set_weights needs a handle created with weights,
        self.w_per_problem = w is not None and w.ndim == 2  # poisson_reweight one with weights per problem
        self.irf_kinds = (not self.external) and any(k in _basis.IRF_KINDS for k in model.kinds)
        if irf is not None:
            if not self.irf_kinds:
                raise ValueError("irf given, but the model has no basis.EXP_DECAY_IRF / basis.IRF function")
            irf = self._as_array(irf)
            _check_irf(irf, self.B, self.m)
        self._grid_step = None
        if self.irf_kinds and not self.device_mode:
            self._grid_step = _uniform_step(x)  # (a device grid is the caller's contract: include/varpro_hip.h)
        self.irf_periodic = (not self.external) and any(k in _basis.PERIODIC_KINDS for k in model.kinds)
        if irf_period is not None:
            irf_period = self._checked_irf_period(irf_period)
        self._keep = (x, Y, w)
        stream = None
        if self.device_mode:
            device = Y.device.index if Y.device.index is not None else torch.cuda.current_device()
            self._tstream = torch.cuda.current_stream(device)  # the handle's stream for its whole life
            stream = C.c_void_p(self._tstream.cuda_stream)
        self.device = int(device)
        h = C.c_void_p()
        eps = -1.0 if epsilon is None else abs(float(epsilon))
        if self.external:
            npairs = len(model.ext_pairs)
            pb = (C.c_int32 * max(1, npairs))(*[j for j, _k in model.ext_pairs])
            pp = (C.c_int32 * max(1, npairs))(*[k for _j, k in model.ext_pairs])
            check(self.lib.vp_batch_create_external(C.byref(h), self.n, self.q, npairs, pb, pp, self.vp_dtype, self.m,
                                                    self.S, self.B, self._ptr(Y), self._ptr(w), eps, flags, self.device,
                                                    stream))
        else:
            desc = model.desc()
            if fixed is not None:
                self._fixed_arg = fixed
                self._create_handle(h, desc, x, Y, w, eps, flags, stream)  # (fixed.py: vp_batch_create_fixed)
            else:
                check(self.lib.vp_batch_create(C.byref(h), C.byref(desc), self.vp_dtype, self.m, self.S, self.B,
                                               self._ptr(x), self._ptr(Y), self._ptr(w), eps, flags, self.device, stream))
        self._h = h
        self._have_params = False  # mirrors the handle: set_params / evaluate / fit has run on the current data
        self._keep = None  # the handle owns copies (Y_w = W*Y, t, w)
        if irf_period is not None:
            self.set_irf_period(irf_period)
        if irf is not None:
            self.set_irf(irf)

    # ---- plumbing ----
    def _as_array(self, a):
        if self.device_mode:
            if not _is_torch(a):
                a = torch.as_tensor(np.asarray(a), device=self._torch_device())
            tdt = torch.float64 if self.np_dtype == np.float64 else torch.float32
            return a.to(dtype=tdt).contiguous()
        return np.ascontiguousarray(a, dtype=self.np_dtype)

    def _torch_device(self):
        return getattr(self, "_tdev", None) or "cuda"

    def _ptr(self, a):
        if a is None:
            return None
        if _is_torch(a):
            self._tdev = a.device
            return C.c_void_p(a.data_ptr())
        return C.c_void_p(a.ctypes.data)

    def _empty(self, shape, dtype=None):
        if self.device_mode:
            if dtype is None:
                tdt = torch.float64 if self.np_dtype == np.float64 else torch.float32
            else:
                tdt = {np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32,
                       np.dtype(np.uint8): torch.uint8}[np.dtype(dtype)]
            return torch.empty(shape, dtype=tdt, device=self._torch_device())
        return np.empty(shape, dtype=self.np_dtype if dtype is None else dtype)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.vp_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _shape_rhs(self, *lead_trail):
        return lead_trail

    # ---- LeastSquaresProblem surface, batch-wise ----
    @_device_entry
    def set_params(self, alpha):
        """== SeparableProblem::set_params (src/solvers/levmar/mod.rs:42-73)"""
        a = self._as_array(alpha).reshape(self.B, self.q)
        check(self.lib.vp_set_params(self._h, self._ptr(a)))
        self._have_params = True

    # ---- caller-evaluated models (model.ExternalModel; vp_batch_create_external) ----
    @_device_entry
    def set_params_with_basis(self, alpha, Phi, dPhi=None):
        """== SeparableProblem::set_params (src/solvers/levmar/mod.rs:42-73) with `model.eval()` replaced by its result:
        Phi (B, n, m) and optionally the derivative columns dPhi (B, p, m), both UNWEIGHTED.  Device tensors are kept by
        POINTER until the next call (keep them alive and unchanged); numpy arrays are copied."""
        a = self._as_array(alpha).reshape(self.B, self.q)
        Phi = self._as_array(Phi).reshape(self.B, self.n, self.m)
        dPhi = None if dPhi is None else self._as_array(dPhi).reshape(self.B, self.p, self.m)
        self._ext_keep = (Phi, dPhi)
        check(self.lib.vp_set_params_with_basis(self._h, self._ptr(a), self._ptr(Phi), self._ptr(dPhi)))
        self._have_params = True

    @_device_entry
    def jacobian_with_derivatives(self, dPhi, with_status=False):
        """== jacobian() (src/solvers/levmar/mod.rs:101-201) with `model.eval_partial_deriv(k)` (:141) replaced by its
        non-zero columns dPhi (B, p, m) at the current parameters"""
        dPhi = self._as_array(dPhi).reshape(self.B, self.p, self.m)
        self._ext_keep = (getattr(self, "_ext_keep", (None, None))[0], dPhi)
        J = self._empty((self.B, self.q, self.S * self.m))
        st = self._empty((self.B,), np.int32)
        check(self.lib.vp_jacobian_with_derivatives(self._h, self._ptr(dPhi), self._ptr(J), self._ptr(st)))
        if not self._have_params:
            J = None
        return (J, st) if with_status else J

    @_device_entry
    def evaluate_with_basis(self, alpha, Phi, dPhi=None, want_residuals=True, want_jacobian=True):
        """fused form (vp_evaluate_with_basis): Phi, dPhi in -> r, J, C, cost, status out in one pass"""
        a = self._as_array(alpha).reshape(self.B, self.q)
        Phi = self._as_array(Phi).reshape(self.B, self.n, self.m)
        dPhi = None if dPhi is None else self._as_array(dPhi).reshape(self.B, self.p, self.m)
        self._ext_keep = (Phi, dPhi)
        want_jacobian = want_jacobian and (dPhi is not None or self.p == 0)
        r = self._empty((self.B, self.S * self.m)) if want_residuals else None
        J = self._empty((self.B, self.q, self.S * self.m)) if want_jacobian else None
        Cm = self._empty((self.B, self.S, self.n))
        cost = self._empty((self.B,), np.float64)
        st = self._empty((self.B,), np.int32)
        check(self.lib.vp_evaluate_with_basis(self._h, self._ptr(a), self._ptr(Phi), self._ptr(dPhi), self._ptr(r),
                                              self._ptr(J), self._ptr(Cm), self._ptr(cost), self._ptr(st)))
        self._have_params = True
        return dict(r=r, J=J, C=Cm.reshape(self.B, self.n) if self.single_rhs else Cm, cost=cost, status=st)

    @_device_entry
    def params(self):
        out = self._empty((self.B, self.q))
        check(self.lib.vp_params(self._h, self._ptr(out)))
        return out

    @_device_entry
    def status(self):
        st = self._empty((self.B,), np.int32)
        check(self.lib.vp_linear_coeffs(self._h, None, self._ptr(st)))
        return st

    @_device_entry
    def residuals(self, with_status=False):
        """== residuals() (src/solvers/levmar/mod.rs:91-95): (B, S*m) column-stacked per problem"""
        r = self._empty((self.B, self.S * self.m))
        st = self._empty((self.B,), np.int32)
        check(self.lib.vp_residuals(self._h, self._ptr(r), self._ptr(st)))
        if not self._have_params:
            r = None  # residuals() before any set_params(): the reference returns None (cached is None)
        return (r, st) if with_status else r

    @_device_entry
    def jacobian(self, with_status=False):
        """== jacobian() (src/solvers/levmar/mod.rs:101-201): (B, q, S*m); J[b, k] is column k"""
        J = self._empty((self.B, self.q, self.S * self.m))
        st = self._empty((self.B,), np.int32)
        check(self.lib.vp_jacobian(self._h, self._ptr(J), self._ptr(st)))
        if not self._have_params:
            J = None  # jacobian() before any set_params(): None, not an uninitialised buffer
        return (J, st) if with_status else J

    @_device_entry
    def linear_coefficients(self):
        """(B, n) for single RHS, (B, S, n) for MRHS (each [b] is the reference's n x S matrix, column-major)"""
        Cm = self._empty((self.B, self.S, self.n))
        check(self.lib.vp_linear_coeffs(self._h, self._ptr(Cm), None))
        return Cm.reshape(self.B, self.n) if self.single_rhs else Cm

    @_device_entry
    def weighted_data(self):
        Yw = self._empty((self.B, self.S, self.m))
        check(self.lib.vp_weighted_data(self._h, self._ptr(Yw)))
        return Yw.reshape(self.B, self.m) if self.single_rhs else Yw

    @_device_entry
    def cost(self):
        c = self._empty((self.B,), np.float64)
        check(self.lib.vp_cost(self._h, self._ptr(c)))
        return c

    @_device_entry
    def evaluate(self, alpha, want_residuals=True, want_jacobian=True):
        """fused set_params + residuals + jacobian + coefficients + cost in one launch (vp_evaluate)"""
        a = self._as_array(alpha).reshape(self.B, self.q)
        r = self._empty((self.B, self.S * self.m)) if want_residuals else None
        J = self._empty((self.B, self.q, self.S * self.m)) if want_jacobian else None
        Cm = self._empty((self.B, self.S, self.n))
        cost = self._empty((self.B,), np.float64)
        st = self._empty((self.B,), np.int32)
        check(self.lib.vp_evaluate(self._h, self._ptr(a), self._ptr(r), self._ptr(J), self._ptr(Cm), self._ptr(cost),
                                   self._ptr(st)))
        self._have_params = True
        return dict(r=r, J=J, C=Cm.reshape(self.B, self.n) if self.single_rhs else Cm, cost=cost, status=st)

    # ---- model surface ----
    @_device_entry
    def basis(self, alpha, skip_invariant=False, want_phi=True, want_dphi=True, out_phi=None, out_dphi=None):
        """== eval / eval_partial_deriv for the batch, UNWEIGHTED (vp_basis): Phi (B, n, m), dPhi (B, p, m)"""
        a = self._as_array(alpha).reshape(self.B, self.q)
        ncols = self.n - (sum(1 for k in self.model.kinds if k == 0) if skip_invariant else 0)
        phi = out_phi if out_phi is not None else (self._empty((self.B, ncols, self.m)) if want_phi else None)
        dphi = out_dphi if out_dphi is not None else (self._empty((self.B, self.p, self.m)) if want_dphi else None)
        check(self.lib.vp_basis(self._h, self._ptr(a), self._ptr(phi), self._ptr(dphi),
                                _lib.VP_BASIS_SKIP_INVARIANT if skip_invariant else 0))
        return phi, dphi

    # ---- solver surface ----
    @_device_entry
    def fit(self, alpha0, solver=None, want_coefficients=True):
        """== LevMarSolver::fit for every problem (vp_fit).  Returns (alpha, C, report) where report
        is a structured numpy array (termination, n_evals, objective); termination > 0 <=> Ok."""
        solver = solver or LevenbergMarquardt(self.np_dtype)
        opts = solver._c()
        a = self._as_array(alpha0).reshape(self.B, self.q)
        a = a.clone() if _is_torch(a) else a.copy()
        Cm = self._empty((self.B, self.S, self.n)) if want_coefficients else None
        if self.device_mode:
            rep_t = torch.empty((self.B, 16), dtype=torch.uint8, device=self._torch_device())
            check(self.lib.vp_fit(self._h, C.byref(opts), self._ptr(a), self._ptr(Cm), self._ptr(rep_t)))
            self._have_params = True  # (only once the call has succeeded: a failed fit leaves the handle without parameters)
            rep = rep_t  # raw bytes on device; use report_to_numpy() to decode
            if Cm is not None and self.single_rhs:
                Cm = Cm.reshape(self.B, self.n)
            return a, Cm, rep
        else:
            rep = np.zeros(self.B, dtype=REPORT_DTYPE)
            check(self.lib.vp_fit(self._h, C.byref(opts), self._ptr(a), self._ptr(Cm), C.c_void_p(rep.ctypes.data)))
            self._have_params = True
        if Cm is not None and self.single_rhs:
            Cm = Cm.reshape(self.B, self.n)
        return a, Cm, rep

    # ---- start-point search (vp_search) ----
    @_device_entry
    def search(self, candidates, per_problem=False):
        """Rank candidate parameter vectors per problem on the device (vp_search) -> ``(alpha (B, q), index (B,) int32,
        cost (B,) float64)``: per problem the candidate with the smallest projected objective 1/2 ||r||^2 (summed over the
        right-hand sides), its index (lowest among equal ones; -1 where no candidate is finite -- alpha is then candidate
        0) and the cost of the evaluation there.  candidates: (K, q) shared by all problems (``candidate_grid`` builds
        one), or (B, K, q) with per_problem=True.  Afterwards the handle is in the state of ``set_params(alpha)``."""
        c = self._as_array(candidates)
        if per_problem:
            if c.ndim != 3 or int(c.shape[0]) != self.B or int(c.shape[2]) != self.q:
                raise ValueError("per-problem candidates must be (B, K, q)")
            K = int(c.shape[1])
        else:
            if c.ndim == 1 and self.q == 1:
                c = c.reshape(-1, 1)
            if c.ndim != 2 or int(c.shape[1]) != self.q:
                raise ValueError("candidates must be (K, q)")
            K = int(c.shape[0])
        a = self._empty((self.B, self.q))
        idx = self._empty((self.B,), np.int32)
        cost = self._empty((self.B,), np.float64)
        check(self.lib.vp_search(self._h, self._ptr(c), K, _lib.VP_SEARCH_PER_PROBLEM if per_problem else 0, self._ptr(a),
                                 self._ptr(idx), self._ptr(cost)))
        self._have_params = True
        return a, idx, cost

    def fit_from_search(self, candidates, solver=None, per_problem=False):
        """``search(candidates)`` then ``fit`` from the winners: (alpha, C, report) as ``fit`` returns them"""
        a, _idx, _cost = self.search(candidates, per_problem=per_problem)
        return self.fit(a, solver)

    def search_stage_ms(self):
        """measurement (include/varpro_hip_debug.h:vp_debug_search_ms): with ``set_timing(True)``, the milliseconds of the
        last shared-route ``search``: [candidate columns, orthonormalisation, ranking product, evaluation at the winners]"""
        ms = (C.c_float * 4)()
        check(self.lib.vp_debug_search_ms(self._h, ms))
        return [float(v) for v in ms]

    # ---- batched fit of a caller-evaluated model by reverse communication (vp_fit_begin / _step_with_basis / _end) ----
    @_device_entry
    def fit_begin(self, alpha0, solver=None, derivatives_on_accept=False):
        """== LevMarSolver::fit (src/solvers/levmar/mod.rs:238-254) for a batch whose model the CALLER evaluates: the
        device keeps one LM driver per problem, the model's columns enter step by step (``fit_step_with_basis``).
        The first step takes the columns at alpha0."""
        solver = solver or LevenbergMarquardt(self.np_dtype)
        opts = solver._c()
        a = self._as_array(alpha0).reshape(self.B, self.q)
        flags = _lib.VP_FIT_DERIVATIVES_ON_ACCEPT if derivatives_on_accept else 0
        check(self.lib.vp_fit_begin(self._h, C.byref(opts), self._ptr(a), flags))
        self._have_params = False
        self._xf_trial = self._empty((self.B, self.q))
        self._xf_want = self._empty((self.B,), np.int32)

    @_device_entry
    def fit_step_with_basis(self, Phi, dPhi=None, want_count=True):
        """one LM iteration of every active problem (vp_fit_step_with_basis): Phi (B, n, m) / dPhi (B, p, m) at the trial
        points of the previous step -> (alpha_trial (B, q), want (B,) int32 of VP_WANT_* bits, n_active or None).
        The returned arrays are REUSED by the next step."""
        Phi = self._as_array(Phi).reshape(self.B, self.n, self.m)
        dPhi = None if dPhi is None else self._as_array(dPhi).reshape(self.B, self.p, self.m)
        self._ext_keep = (Phi, dPhi)
        nact = C.c_int64(0)
        check(self.lib.vp_fit_step_with_basis(self._h, self._ptr(Phi), self._ptr(dPhi), self._ptr(self._xf_trial),
                                              self._ptr(self._xf_want), C.byref(nact) if want_count else None))
        return self._xf_trial, self._xf_want, (int(nact.value) if want_count else None)

    @_device_entry
    def fit_active_set(self, index_out=None, count_out=None):
        """the compacted active set of the running stepped fit (vp_fit_active_set): ``(index (B,) int32, count (1,) int32)`` --
        index[:count] are the problems still running; entries beyond are stale but valid indices.  Device-pointer handles:
        torch tensors filled asynchronously (no synchronisation); pass the previous call's tensors to reuse them."""
        idx = index_out if index_out is not None else self._empty((self.B,), np.int32)
        cnt = count_out if count_out is not None else self._empty((1,), np.int32)
        check(self.lib.vp_fit_active_set(self._h, self._ptr(idx), self._ptr(cnt)))
        return idx, cnt

    @_device_entry
    def fit_end(self, want_coefficients=True):
        """(alpha, C, report) of the stepped fit (vp_fit_end); report as ``fit`` returns it"""
        a = self._empty((self.B, self.q))
        Cm = self._empty((self.B, self.n) if self.single_rhs else (self.B, self.S, self.n)) if want_coefficients else None
        if self.device_mode:
            rep = torch.empty((self.B, 16), dtype=torch.uint8, device=self._torch_device())
            check(self.lib.vp_fit_end(self._h, self._ptr(a), self._ptr(Cm), self._ptr(rep)))
        else:
            rep = np.zeros(self.B, dtype=REPORT_DTYPE)
            check(self.lib.vp_fit_end(self._h, self._ptr(a), self._ptr(Cm), C.c_void_p(rep.ctypes.data)))
        self._have_params = True
        return a, Cm, rep

    def fit_with_model(self, evaluate, alpha0, solver=None, derivatives_on_accept=False, max_steps=None, check_every=1):
        """The whole stepped fit: ``evaluate(alpha (B, q), want (B,) or None) -> (Phi, dPhi)`` is the caller's model (numpy
        on host-pointer handles, torch on device-pointer handles; ``want`` is None for the first call, afterwards the
        VP_WANT_* bits per problem -- entries of problems that want nothing are never read, a model may skip them).
        Returns (alpha, C, report, steps)."""
        self.fit_begin(alpha0, solver, derivatives_on_accept)
        solver = solver or LevenbergMarquardt(self.np_dtype)
        limit = max_steps if max_steps is not None else 2 * (solver.patience * (self.q + 1) + 2)
        alpha, want = self._as_array(alpha0).reshape(self.B, self.q), None
        steps = 0
        while steps < limit:
            Phi, dPhi = evaluate(alpha, want)
            steps += 1
            look = (steps % check_every == 0) or steps == limit
            alpha, want, nact = self.fit_step_with_basis(Phi, dPhi, want_count=look)
            if look and nact == 0:
                break
        a, Cm, rep = self.fit_end()
        return a, Cm, rep, steps

    def fit_trace(self, alpha0, solver=None, max_rows=512):
        """diagnostics (host mode only): fit + per-evaluation trace (B, max_rows, q+4) with rows
        [alpha_trial, ||r||, ratio, delta, par]; unused rows are NaN"""
        assert not self.device_mode
        solver = solver or LevenbergMarquardt(self.np_dtype)
        opts = solver._c()
        a = self._as_array(alpha0).reshape(self.B, self.q).copy()
        Cm = self._empty((self.B, self.S, self.n))
        rep = np.zeros(self.B, dtype=REPORT_DTYPE)
        tr = np.zeros((self.B, max_rows, self.q + 4))
        check(self.lib.vp_fit_trace(self._h, C.byref(opts), self._ptr(a), self._ptr(Cm), C.c_void_p(rep.ctypes.data),
                                    C.c_void_p(tr.ctypes.data), int(max_rows)))
        self._have_params = True
        if self.single_rhs:
            Cm = Cm.reshape(self.B, self.n)
        return a, Cm, rep, tr

    @staticmethod
    def report_to_numpy(rep):
        if _is_torch(rep):
            return rep.cpu().numpy().view(REPORT_DTYPE).reshape(-1)
        return rep

    @_device_entry
    def debug_gram_evaluate(self, alpha):
        """diagnostics (vp_debug_gram_evaluate): the fp64-Gram fit kernel's formulation evaluated once at alpha ->
        dict(cost (B,), C (B, n), Jtr (B, q), JtJ (B, q, q)), all float64"""
        a = self._as_array(alpha).reshape(self.B, self.q)
        per = 1 + self.n + self.q + self.q * self.q
        out = self._empty((self.B, per), np.float64)
        check(self.lib.vp_debug_gram_evaluate(self._h, self._ptr(a), self._ptr(out)))
        n, q = self.n, self.q
        return dict(cost=out[:, 0], C=out[:, 1:1 + n], Jtr=out[:, 1 + n:1 + n + q],
                    JtJ=out[:, 1 + n + q:].reshape(self.B, q, q))

    def kernel_set(self):
        """test hook (vp_debug_kernel_set): the compiled kernel set this handle runs on, the tuple _lib.KERNEL_SET_FIELDS
        = (dtype, family, a, b, c, R, W, uses_gen_ws)"""
        rec = (C.c_int32 * 8)()
        check(self.lib.vp_debug_kernel_set(self._h, rec))
        return tuple(int(v) for v in rec)

    def last_fit_kernel(self):
        """test hook (vp_debug_last_fit): (kernel, padding, weighted, 0) of the launch the last fit issued -- kernel 0 = no fit
        yet, 1 = wave, 2 = slots, 3 = Gram (fp32 handle, fp64 Gram matrix), 4 = row-block, 5 = generic; padding 1 = m fills the set, 2 = last register pair,
        0 = general, -1 = not applicable"""
        rec = (C.c_int32 * 4)()
        check(self.lib.vp_debug_last_fit(self._h, rec))
        return tuple(int(v) for v in rec)

    def last_global_launch(self):
        """test hook (vp_debug_last_global): (factor_waves, step_waves, fit_stream, eval_stream, gx_fit, gx_eval, 0, 0) of the
        launches the handle's global fits and evaluations (several right-hand sides) issued -- waves 1 or 4 per problem, 0 =
        not launched yet; stream 0 = none yet, 1 = streaming kernel, 2 = cooperative DMA kernel, 3 / 4 = cooperative output
        kernel with / without J, 5 = the generic kernels; gx workgroups per problem of that pass"""
        rec = (C.c_int32 * 8)()
        check(self.lib.vp_debug_last_global(self._h, rec))
        return tuple(int(v) for v in rec)

    @_device_entry
    def best_fit(self):
        """== FitResult::best_fit (src/fit.rs:55-59, 87-91)"""
        f = self._empty((self.B, self.S, self.m))
        check(self.lib.vp_best_fit(self._h, self._ptr(f)))
        return f.reshape(self.B, self.m) if self.single_rhs else f

    @_device_entry
    def statistics(self, want_confidence_sigma=True):
        """== FitStatistics::try_calculate for every problem (vp_statistics): dict(cov (B,k,k),
        reduced_chi2 (B,), conf_sigma (B,m) or None, status (B,), dof)"""
        k = self.n + self.q
        cov = self._empty((self.B, k, k))
        chi2 = self._empty((self.B,), np.float64)
        sig = self._empty((self.B, self.m)) if want_confidence_sigma else None
        st = self._empty((self.B,), np.int32)
        check(self.lib.vp_statistics(self._h, self._ptr(cov), self._ptr(chi2), self._ptr(sig), self._ptr(st)))
        return dict(cov=cov, reduced_chi2=chi2, conf_sigma=sig, status=st, dof=self.m - k)

    @_device_entry
    def global_statistics(self, want_coef_cov=True, want_confidence_sigma=False):
        """Fit statistics of a global fit (any S >= 1; vp_global_statistics): FitStatistics::try_calculate on the stacked
        single-RHS problem (m S observations, parameters [c_1 .. c_S, alpha]) -> dict(cov_alpha (B,q,q), reduced_chi2 (B,),
        coef_cov (B,S,n,n) and coef_alpha_cov (B,S,n,q) or None, conf_sigma (B,S,m) or None, status (B,),
        dof = m S - n S - q).  The cross blocks Cov(c_s, c_t), s != t, are not produced."""
        B, S, n, q, m = self.B, self.S, self.n, self.q, self.m
        cov = self._empty((B, q, q))
        chi2 = self._empty((B,), np.float64)
        cc = self._empty((B, S, n, n)) if want_coef_cov else None
        ca = self._empty((B, S, n, q)) if want_coef_cov else None
        sig = self._empty((B, S, m)) if want_confidence_sigma else None
        st = self._empty((B,), np.int32)
        check(self.lib.vp_global_statistics(self._h, self._ptr(cov), self._ptr(chi2), self._ptr(cc), self._ptr(ca),
                                            self._ptr(sig), self._ptr(st)))
        return dict(cov_alpha=cov, reduced_chi2=chi2, coef_cov=cc, coef_alpha_cov=ca, conf_sigma=sig, status=st,
                    dof=m * S - n * S - q)

    @_device_entry
    def set_observations(self, Y):
        """replace the data of this handle by another batch of the same shape (vp_set_observations): the next frame
        of a stream of same-shaped problems without re-allocating the device state"""
        Y = self._as_array(Y)
        want = (self.B, self.m) if self.single_rhs else (self.B, self.S, self.m)
        if tuple(Y.shape) != want:
            raise ValueError("observations must have shape %r" % (want,))
        if self.device_mode and not Y.is_contiguous():
            Y = Y.contiguous()
        check(self.lib.vp_set_observations(self._h, self._ptr(Y)))
        self._have_params = False

    # ---- weights between fits; Poisson-weighted fits (vp_set_weights, vp_poisson_reweight) ----
    def _checked_observations(self, Y, what):
        Y = self._as_array(Y)
        want = (self.B, self.m) if self.single_rhs else (self.B, self.S, self.m)
        if tuple(Y.shape) != want:
            raise ValueError("%s: observations must have shape %r" % (what, want))
        return Y

    @_device_entry
    def set_weights(self, w, Y):
        """replace the weights of a handle that was created with weights (vp_set_weights): w in the layout of creation,
        (m,) or (B, m); Y the observations again -- the handle keeps only W Y, so the new weighted data is formed from
        them.  Cached results are invalidated, as by ``set_observations``."""
        if not self.weighted:
            raise ValueError("set_weights: the handle was created without weights (unit-weight handles run on other kernels)")
        w = self._as_array(w)
        if tuple(w.shape) != ((self.B, self.m) if self.w_per_problem else (self.m,)):
            raise ValueError("set_weights: the weights keep the layout of creation, %s"
                             % ("(B, m)" if self.w_per_problem else "(m,)"))
        Y = self._checked_observations(Y, "set_weights")
        check(self.lib.vp_set_weights(self._h, self._ptr(w), self._ptr(Y)))
        self._have_params = False

    @_device_entry
    def poisson_reweight(self, Y, mode="model", floor=1.0):
        """Weights of Poisson counts Y (B, m), formed on the device (vp_poisson_reweight): w = 1/sqrt(max(v, floor)) with
        v = Y (mode "neyman") or v = the handle's current best fit (mode "model": after ``fit`` / ``set_params``).  The
        handle's weights and weighted data are replaced, cached results are invalidated, ``params()`` still returns the
        parameters.  "model" returns ``(deviance, pearson)``, both (B,) float64 -- the Poisson deviance
        2 sum [y ln(y/f) - (y - f)] and Pearson's X^2 = sum (y - f)^2 / f of the fit the weights were formed from (NaN for a
        problem whose evaluation failed; its weights are kept) -- and "neyman" returns None.  Needs a single right-hand
        side and a handle created with per-problem weights (``weights="neyman"`` or a (B, m) array)."""
        if mode not in ("neyman", "model"):
            raise ValueError("poisson_reweight: mode is \"neyman\" or \"model\"")
        floor = float(floor)
        if not (np.isfinite(floor) and floor > 0.0):
            raise ValueError("poisson_reweight: the floor must be finite and > 0")
        if not self.single_rhs:
            raise ValueError("poisson_reweight: weights are per problem, not per right-hand side (S = 1 only)")
        if not self.w_per_problem:
            raise ValueError("poisson_reweight: the handle needs per-problem weights (weights=\"neyman\" or a (B, m) array)")
        Y = self._checked_observations(Y, "poisson_reweight")
        if mode == "model" and not self._have_params:
            raise ValueError("poisson_reweight: mode \"model\" needs the fit of the current parameters (fit / set_params first)")
        dev = pear = None
        if mode == "model":
            dev, pear = self._empty((self.B,), np.float64), self._empty((self.B,), np.float64)
        check(self.lib.vp_poisson_reweight(self._h, self._ptr(Y), _lib.VP_POISSON_MODEL if mode == "model" else
                                           _lib.VP_POISSON_NEYMAN, C.c_double(floor), self._ptr(dev), self._ptr(pear)))
        self._have_params = False
        return (dev, pear) if mode == "model" else None

    def fit_poisson(self, counts, alpha0, rounds=POISSON_ROUNDS, floor=1.0, solver=None):
        """Poisson maximum-likelihood fit of counts (B, m) by iterated re-weighting: a Neyman-weighted fit from alpha0, then
        ``rounds`` fits with the weights 1/sqrt(max(f, floor)) of the previous fit, each from the previous parameters -- the
        fixed point of which is the Poisson score equations.  One more model re-weight and an evaluation end it, so the
        returned ``(alpha, C, report, info)`` carries ``info = dict(deviance, pearson, reduced_deviance, rounds)`` AT the
        returned point and the handle's state is that point (``statistics()``, ``best_fit()`` need no further call; the
        statistics are those of the weighted least-squares problem at the final weights, i.e. the Fisher-information
        covariance at the estimate).  report is the last fit's.  ``rounds`` is a fixed count: a device-pointer handle makes
        no host visit between the rounds."""
        rounds = int(rounds)
        if rounds < 0:
            raise ValueError("fit_poisson: rounds >= 0")
        self.poisson_reweight(counts, "neyman", floor)
        a, Cm, rep = self.fit(alpha0, solver)
        for _ in range(rounds):
            self.poisson_reweight(counts, "model", floor)
            a, Cm, rep = self.fit(a, solver)
        # deviance and X^2 of the returned (alpha, C); the evaluation makes the handle's state that alpha at the final weights
        # (its coefficients differ from C by what one more round would change: nothing beyond the fits' own stopping noise)
        dev, pear = self.poisson_reweight(counts, "model", floor)
        self.evaluate(a, want_residuals=False, want_jacobian=False)
        info = dict(deviance=dev, pearson=pear, reduced_deviance=dev / float(self.m - self.n - self.q), rounds=rounds)
        return a, Cm, rep, info

    # ---- robust fits (vp_robust_reweight, vp_weights) ----
    @_device_entry
    def weights(self):
        """the handle's current weights (vp_weights), (m,) or (B, m) as created; after ``robust_reweight`` /
        ``fit_robust`` they are the outlier map of the fit (a weight far below its base weight marks an outlier)"""
        if not self.weighted:
            raise ValueError("weights: the handle was created without weights")
        w = self._empty((self.B, self.m) if self.w_per_problem else (self.m,))
        check(self.lib.vp_weights(self._h, self._ptr(w)))
        return w

    def _robust_arguments(self, loss, tuning, scale, what):
        if loss not in ROBUST_LOSSES:
            raise ValueError("%s: loss is \"huber\", \"cauchy\" or \"tukey\"" % what)
        tuning = 0.0 if tuning is None else float(tuning)
        if tuning != 0.0 and not (np.isfinite(tuning) and tuning > 0.0):
            raise ValueError("%s: the tuning constant must be finite and > 0 (None: the 95 %% efficiency value)" % what)
        scale = 0.0 if scale is None else float(scale)
        if scale != 0.0 and not (np.isfinite(scale) and scale > 0.0):
            raise ValueError("%s: the scale must be finite and > 0 (None: the normalised median of |e| per problem)" % what)
        if not self.single_rhs:
            raise ValueError("%s: weights are per problem, not per right-hand side (S = 1 only)" % what)
        if not self.w_per_problem:
            raise ValueError("%s: the handle needs per-problem weights (weights=\"unit\", \"neyman\" or a (B, m) array)" % what)
        return ROBUST_LOSSES[loss], tuning, scale

    def _checked_base_weights(self, w0, what):
        if w0 is None:
            return None
        w0 = self._as_array(w0)
        if tuple(w0.shape) != (self.B, self.m):
            raise ValueError("%s: the base weights must have shape %r" % (what, (self.B, self.m)))
        return w0

    @_device_entry
    def robust_reweight(self, Y, loss="huber", tuning=None, scale=None, base_weights=None):
        """M-estimator weights from the residuals of the handle's current best fit, formed on the device
        (vp_robust_reweight): w = w0 sqrt(omega(u)), u = w0 (y - f)/s, with omega of ``loss`` "huber", "cauchy" or "tukey"
        and the tuning constant ``tuning`` (None: 1.345 / 2.385 / 4.685, 95 % efficiency on normal data).  ``scale`` None
        estimates s per problem as 1.4826 times the median of |w0 (y - f)| over the rows with w0 != 0; a number fixes it
        for the batch (the choice when w0 = 1/sigma is known).  ``base_weights`` (B, m) are w0 (None: 1) -- they should
        make the residuals of the clean data homoscedastic (Neyman weights for counts: with unit weights on Poisson data
        the median is set by the tail and the peak passes for an outlier) -- and are passed again every round, because
        the handle's own weights are replaced.  Needs the fit of the current parameters (after ``fit`` / ``set_params``),
        a single right-hand side and a handle with per-problem weights.  Cached results are invalidated, ``params()``
        still returns the parameters.  Returns ``(scale, rho)``, both (B,) float64: s and sum rho(u) of the fit the weights
        were formed from (NaN for a problem whose evaluation failed; its weights are kept)."""
        loss, tuning, scale = self._robust_arguments(loss, tuning, scale, "robust_reweight")
        Y = self._checked_observations(Y, "robust_reweight")
        w0 = self._checked_base_weights(base_weights, "robust_reweight")
        if not self._have_params:
            raise ValueError("robust_reweight needs the fit of the current parameters (fit / set_params first)")
        s, rho = self._empty((self.B,), np.float64), self._empty((self.B,), np.float64)
        check(self.lib.vp_robust_reweight(self._h, self._ptr(Y), self._ptr(w0), loss, C.c_double(tuning), C.c_double(scale),
                                          self._ptr(s), self._ptr(rho)))
        self._have_params = False
        return s, rho

    def fit_robust(self, Y, alpha0, loss="huber", tuning=None, scale=None, rounds=ROBUST_ROUNDS, base_weights=None, solver=None):
        """Robust (M-estimator) fit of Y (B, m) by iterated re-weighting -- not a Levenberg-Marquardt on rho: a fit at the
        base weights from alpha0, then ``rounds`` times {``robust_reweight``, a fit from the previous parameters}, the
        fixed point of which is the estimating equations sum psi(u_i) w0_i df_i/dtheta = 0.  One more re-weight and an
        evaluation end it, so the returned ``(alpha, C, report, info)`` carries ``info = dict(scale, rho, rounds, weights)``
        AT the returned point -- ``weights`` is the outlier map that belongs to it -- and the handle's state is that point
        (``statistics()``, ``best_fit()`` need no further call).  ``statistics()`` is then the covariance of the weighted
        least-squares problem at the final weights, not a sandwich estimator.  "huber" is convex; "tukey" and "cauchy" are
        not and need a start from a sensible fit (alpha0 from a plain or a Huber fit).  ``base_weights`` None: unit weights;
        see ``robust_reweight`` for what they should be.  ``rounds`` is a fixed count: a device-pointer handle makes no
        host visit between the rounds, and torch tensors stay on the device throughout."""
        rounds = int(rounds)
        if rounds < 0:
            raise ValueError("fit_robust: rounds >= 0")
        self._robust_arguments(loss, tuning, scale, "fit_robust")
        Y = self._checked_observations(Y, "fit_robust")
        w0 = self._checked_base_weights(base_weights, "fit_robust")
        if w0 is None:
            w0 = torch.ones_like(Y) if self.device_mode else np.ones_like(Y)
        self.set_weights(w0, Y)
        a, Cm, rep = self.fit(alpha0, solver)
        for _ in range(rounds):
            self.robust_reweight(Y, loss, tuning, scale, w0)
            a, Cm, rep = self.fit(a, solver)
        # scale, rho and the weights of the returned (alpha, C); the evaluation makes the handle's state that alpha at them
        s, rho = self.robust_reweight(Y, loss, tuning, scale, w0)
        self.evaluate(a, want_residuals=False, want_jacobian=False)
        return a, Cm, rep, dict(scale=s, rho=rho, rounds=rounds, weights=self.weights())

    @_device_entry
    def set_irf(self, irf):
        """the instrument response of a model with ``basis.EXP_DECAY_IRF`` / ``basis.IRF`` (vp_set_irf): (m,) shared by the
        batch or (B, m); the handle copies it (torch tensors: on the device, on the handle's stream).  May be called again
        to replace the response -- with ``set_observations`` for the next frame; cached results are invalidated."""
        if not self.irf_kinds:
            raise ValueError("set_irf: the model has no basis.EXP_DECAY_IRF / basis.IRF function")
        irf, per_problem = _check_irf(self._as_array(irf), self.B, self.m)
        check(self.lib.vp_set_irf(self._h, self._ptr(irf), int(per_problem)))
        self._have_params = False

    def _checked_irf_period(self, period):
        if not self.irf_periodic:
            raise ValueError("irf_period: the model has no basis.EXP_DECAY_IRF_PERIODIC function")
        return _check_irf_period(period, self.m, self._grid_step)

    @_device_entry
    def set_irf_period(self, period):
        """the period T of ``basis.EXP_DECAY_IRF_PERIODIC`` in the units of the grid, shared by the batch
        (vp_set_irf_period); None or 0: the record is exactly one period, T = m dt per grid.  ValueError: NaN, a negative
        value, a model without the kind, a host grid with T < m dt.  Cached results are invalidated."""
        period = self._checked_irf_period(period)
        check(self.lib.vp_set_irf_period(self._h, C.c_double(period)))
        self._have_params = False

    def set_bounds(self, lower, upper):
        """Box bounds on the nonlinear parameters of ``fit`` (vp_set_bounds; device-column handles: a model with a peak /
        baseline kind, or ``device_columns=True``).  lower / upper: arrays of shape (q,) or (B, q); None on a side or an
        infinite entry means unbounded; ``set_bounds(None, None)`` clears.  The bounds stay set across ``fit`` and
        ``set_observations``.  The fit iterates on internal parameters (varpro_amd.bounds): every returned parameter lies
        inside its box, the tolerances of the solver act on the internal parameters, and a start on a bound stays there --
        start strictly inside.  ValueError: wrong shape, NaN, lower >= upper."""
        nb = _bounds.normalize(None if lower is None else np.asarray(_to_host(lower), dtype=np.float64),
                               None if upper is None else np.asarray(_to_host(upper), dtype=np.float64), self.B, self.q)
        if nb is None:
            check(self.lib.vp_set_bounds(self._h, None, None, 0))
            return
        lo, hi, per_problem = nb
        dp = C.POINTER(C.c_double)
        check(self.lib.vp_set_bounds(self._h, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), int(per_problem)))

    def set_rhs_allreduce(self, global_rhs_count, group=None):
        """Shard ONE global fit over ranks by right-hand sides (vp_set_rhs_allreduce): this handle
        holds the local block of the S columns (torch device tensors); per LM evaluation the B*(1+n*n+p) reduced
        sums are all-reduced over `group` (torch.distributed: backend "nccl" == RCCL over xGMI; "gloo" is bounced
        through the host and only meant for tests).  Pass global_rhs_count=None to switch back."""
        if global_rhs_count is None:
            self._rhs_cb = None
            check(self.lib.vp_set_rhs_allreduce(self._h, _lib.ALLREDUCE_FN(0), None, 0))
            return
        if not self.device_mode:
            raise ValueError("right-hand-side sharding needs device tensors (the collective runs on the stream)")
        import torch
        import torch.distributed as dist

        dev = self._tdev

        class _Raw:  # zero-copy view of the library's device buffer for torch
            def __init__(self, ptr, count):
                self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": "<f8", "data": (int(ptr), False),
                                                 "version": 2}

        def _cb(ptr, count, stream, user):
            try:
                # the library hands over the stream its kernels run on: the collective must be ordered on THAT
                # stream (after the partial-sum kernel, before the LM step), whatever torch's current stream is
                sptr = int(stream) if stream else 0
                lib_stream = torch.cuda.ExternalStream(sptr, device=dev) if sptr else torch.cuda.default_stream(dev)
                with torch.cuda.stream(lib_stream):
                    t = torch.as_tensor(_Raw(ptr, count), device=dev)
                    if dist.get_backend(group) == "gloo":
                        h = t.cpu()
                        dist.all_reduce(h, group=group)
                        t.copy_(h)
                    else:
                        dist.all_reduce(t, group=group)
                return 0
            except Exception as e:  # never let an exception cross the C boundary
                self._rhs_cb_error = e
                return -1

        self._rhs_cb = _lib.ALLREDUCE_FN(_cb)  # keep alive as long as the handle uses it
        check(self.lib.vp_set_rhs_allreduce(self._h, self._rhs_cb, None, int(global_rhs_count)))

    @_device_entry
    def summary(self):
        """local {sum cost, #successful, #failed, sum n_evals} after fit (vp_summary)"""
        out = (C.c_double * 4)()
        check(self.lib.vp_summary(self._h, out))
        return np.array(list(out))

    @_device_entry
    def global_fit_condition(self):
        """(B,) largest estimate of cond(J D^-1) the Gram-based LM steps of the last GLOBAL fit (S > 1) have seen
        (vp_global_fit_condition): the step is exact to ~10 cond^2 eps -- beyond ~1e5 it is at rounding level"""
        out = self._empty((self.B,), np.float64)
        check(self.lib.vp_global_fit_condition(self._h, self._ptr(out)))
        return out

    @_device_entry
    def summary_device(self, out):
        """the same 4 aggregates into a CUDA float64 tensor of 4 elements, asynchronously on the handle's stream
        (no host synchronisation): ready to be all-reduced over RCCL"""
        assert _is_torch(out) and out.is_cuda and out.numel() == 4 and out.dtype == torch.float64
        check(self.lib.vp_summary_device(self._h, C.c_void_p(out.data_ptr())))
        return out

    def set_fit_kernel(self, which):
        """single-RHS fit kernel selection: "auto" | "wave" (one wavefront per problem) | "slots" (persistent
        slot kernel wherever it covers the problem) -- see include/varpro_hip.h:vp_set_fit_kernel"""
        code = {"auto": _lib.VP_FIT_KERNEL_AUTO, "wave": _lib.VP_FIT_KERNEL_WAVE, "slots": _lib.VP_FIT_KERNEL_SLOTS}[which]
        check(self.lib.vp_set_fit_kernel(self._h, code))

    def set_refit(self, enable=True):
        """diagnostics (include/varpro_hip_debug.h:vp_debug_set_refit): False returns what the fit kernels themselves report
        for a problem whose Jacobian factor is not representable column by column (Numerical, parameters = the guess)
        instead of re-fitting it with scaled columns in vp_fit's second launch"""
        check(self.lib.vp_debug_set_refit(self._h, int(enable)))

    def set_column_fit(self, look_every=8, nontemporal=1):
        """measurement switches of a handle whose model has a peak / baseline kind (include/varpro_hip_debug.h:
        vp_debug_set_column_fit): the step interval at which ``fit`` reads the active count, and the column kernel's store mode"""
        check(self.lib.vp_debug_set_column_fit(self._h, int(look_every), int(nontemporal)))

    def set_timing(self, enable=True):
        check(self.lib.vp_set_timing(self._h, int(enable)))

    def last_kernel_ms(self, which):
        ms = C.c_float(-1.0)
        check(self.lib.vp_last_kernel_ms(self._h, int(which), C.byref(ms)))
        return float(ms.value)

    def synchronize(self):
        check(self.lib.vp_synchronize(self._h))
