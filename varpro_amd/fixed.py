"""Fixed nonlinear parameters: ``BatchProblem(model, Y, fixed={"tau2": 2.5})`` (vp_batch_create_fixed).

The device handle of such a problem IS the reduced model: it knows the free parameters only, in model order, and only
its column kernels see the full parameter vector (include/varpro_hip.h).  The Python mirror stays in the FULL parameter
order: this module holds the bookkeeping between the two -- the mask and the values from the user's dict, the reduction
of full-order inputs to the free columns, the expansion of the handle's answers and the scatter of a covariance -- as
plain functions on arrays (tested without a device), and ``FixedBatchProblem``, the subclass ``BatchProblem(...,
fixed=...)`` constructs.  A problem without ``fixed`` never comes here.
"""
import ctypes as C

import numpy as np

from ._lib import check
from .batch import BatchProblem, _device_entry, _is_torch, _to_host

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


def fixed_mask(parameter_names, fixed):
    """``fixed``: dict name -> value.  Returns (mask (q,) int32 of 0 / 1, free (q_free,) intp, held (q - q_free,) intp);
    ValueError: not a dict, an unknown name, no free parameter left"""
    names = list(parameter_names)
    if not isinstance(fixed, dict):
        raise ValueError("fixed: a dict of parameter name -> value")
    unknown = [k for k in fixed if k not in names]
    if unknown:
        raise ValueError("fixed: unknown parameter name(s) %r (the model's parameters are %r)" % (unknown, names))
    mask = np.array([1 if n in fixed else 0 for n in names], dtype=np.int32)
    if names and int(mask.sum()) == len(names):
        raise ValueError("fixed: no free parameter left")
    return mask, np.flatnonzero(mask == 0), np.flatnonzero(mask == 1)


def fixed_values(parameter_names, fixed, B):
    """the values of ``fixed`` as float64: (q,) when every value is a scalar, else (B, q) (a value is a scalar or a (B,)
    array); entries of free parameters are 0.  Returns (values, per_problem).  ValueError: a value of another shape"""
    names = list(parameter_names)
    vals = {k: np.asarray(_to_host(v), dtype=np.float64) for k, v in fixed.items()}
    for k, v in vals.items():
        if v.ndim == 1 and v.shape[0] == 1 and B != 1:
            vals[k] = v.reshape(())
        elif not (v.ndim == 0 or v.shape == (B,)):
            raise ValueError("fixed[%r]: a scalar or an array of shape (%d,), got %r" % (k, B, v.shape))
    per_problem = any(v.ndim == 1 for v in vals.values())
    out = np.zeros((B, len(names)) if per_problem else (len(names),), dtype=np.float64)
    for k, v in vals.items():
        out[..., names.index(k)] = v
    return out, per_problem


def _index(idx, like):
    """``idx`` as an index for ``like``: a device tensor for a torch array (one that is already there is used as it is -- the
    handle keeps its own, so that a call makes no host-to-device copy), else a numpy array"""
    if _is_torch(like):
        return idx if _is_torch(idx) else torch.as_tensor(np.asarray(idx), device=like.device)
    return np.asarray(_to_host(idx))


def reduce_columns(a, free):
    """the columns of the free parameters of a full-order array (..., q) (numpy or torch), in model order"""
    if _is_torch(a):
        return a[..., _index(free, a)].contiguous()
    return np.ascontiguousarray(a[..., _index(free, a)])


def expand_columns(a_free, free, held, values, q):
    """full-order (B, q) from the handle's (B, q_free): free columns from ``a_free``, held ones from ``values`` ((q,) or
    (B, q), rounded to the dtype of ``a_free`` as the kernels read them)"""
    B = int(a_free.shape[0])
    if _is_torch(a_free):
        out = torch.empty((B, q), dtype=a_free.dtype, device=a_free.device)
        out[:, _index(free, a_free)] = a_free
        if len(held):
            hi = _index(held, a_free)
            v = values if _is_torch(values) else torch.as_tensor(values, device=a_free.device)
            out[:, hi] = v[..., hi].to(a_free.dtype).expand(B, len(held))
        return out
    out = np.empty((B, q), dtype=a_free.dtype)
    free, held = _index(free, a_free), _index(held, a_free)
    out[:, free] = a_free
    if len(held):
        out[:, held] = np.asarray(_to_host(values))[..., held].astype(a_free.dtype)
    return out


def scatter_square(c_free, index, size):
    """(B, k, k) over the kept rows / columns ``index`` -> (B, size, size) with exact zeros elsewhere"""
    B = int(c_free.shape[0])
    if _is_torch(c_free):
        out = torch.zeros((B, size, size), dtype=c_free.dtype, device=c_free.device)
        ix = torch.as_tensor(np.asarray(index), device=c_free.device)
        out[:, ix[:, None], ix[None, :]] = c_free
        return out
    out = np.zeros((B, size, size), dtype=c_free.dtype)
    out[:, np.asarray(index)[:, None], np.asarray(index)[None, :]] = c_free
    return out


def scatter_last(c_free, index, size):
    """(..., k) over the kept last-axis entries ``index`` -> (..., size) with exact zeros elsewhere"""
    if _is_torch(c_free):
        out = torch.zeros(tuple(c_free.shape[:-1]) + (size,), dtype=c_free.dtype, device=c_free.device)
        out[..., torch.as_tensor(np.asarray(index), device=c_free.device)] = c_free
        return out
    out = np.zeros(tuple(c_free.shape[:-1]) + (size,), dtype=c_free.dtype)
    out[..., np.asarray(index)] = c_free
    return out


class FixedBatchProblem(BatchProblem):
    """``BatchProblem(model, Y, fixed={name: value})``: the named nonlinear parameters are held at their values (a scalar,
    or a (B,) array / tensor: one value per problem) and not fitted.  Everything is in the model's FULL parameter order:

    - ``fit(alpha0)``, ``set_params``, ``evaluate``, ``basis``, ``search`` and ``set_bounds`` take (q,)- / (B, q)-shaped
      input whose columns of fixed parameters are ignored; ``fit``, ``search`` and ``params`` return the full alpha with the
      fixed entries filled in;
    - ``statistics()`` / ``global_statistics()`` return the covariance in full size with exact zeros in the rows and
      columns of fixed parameters, plus ``"free"``: the indices of the free nonlinear parameters.  It is the covariance of
      the problem that was solved (dof counts the free parameters);
    - derivative-shaped results -- ``jacobian()``, ``evaluate()["J"]``, the dPhi of ``basis()`` -- have the columns of the
      free parameters only, in model order; ``residuals``, ``best_fit`` and ``conf_sigma`` keep their shapes;
    - ``set_fixed(name=value)`` replaces values between fits (a profile-likelihood scan); the mask cannot change.

    ``q`` and ``p`` are those of the handle (free parameters and their derivative columns), ``q_full`` the model's."""

    def __init__(self, model, Y, *args, **kwargs):
        if kwargs.get("fixed") is None:
            raise ValueError("FixedBatchProblem needs fixed={name: value} ({}: nothing held); without it construct BatchProblem")
        super().__init__(model, Y, *args, **kwargs)

    def _create_handle(self, h, desc, x, Y, w, eps, flags, stream):
        mask, self.free, self.held = fixed_mask(self.model.parameter_names, self._fixed_arg)
        self.q_full = self.q
        self.q = int(self.free.size)
        self.p = sum(1 for _j, _a, pi in self.model.pairs if mask[pi] == 0)
        self._fixed = dict(self._fixed_arg)
        vals, per = self._fixed_array()
        cm = (C.c_int32 * max(1, self.q_full))(*[int(v) for v in mask])
        check(self.lib.vp_batch_create_fixed(C.byref(h), C.byref(desc), self.vp_dtype, self.m, self.S, self.B, self._ptr(x),
                                             self._ptr(Y), self._ptr(w), eps, flags, self.device, stream, cm,
                                             self._ptr(vals), int(per)))
        self._fix_values = vals
        # device mode: the index tensors live on the device once, and nothing held means nothing to gather or scatter
        self._free_ix, self._held_ix = self.free, self.held
        if self.device_mode:
            self._free_ix = torch.as_tensor(self.free, device=self._torch_device())
            self._held_ix = torch.as_tensor(self.held, device=self._torch_device())

    def _fixed_array(self):
        """the current values as the library takes them: float64 (q,) or (B, q), on the device in device mode"""
        if self.device_mode:  # built with torch: a device tensor among the values makes no host visit
            per = self.B != 1 and any((v.ndim if _is_torch(v) else np.ndim(v)) == 1 and len(v) == self.B for v in self._fixed.values())
            out = torch.zeros((self.B, self.q_full) if per else (self.q_full,), dtype=torch.float64, device=self._torch_device())
            for k, v in self._fixed.items():
                v = v if _is_torch(v) else torch.as_tensor(np.asarray(v, dtype=np.float64))
                v = v.to(device=out.device, dtype=torch.float64)
                if not (v.ndim == 0 or tuple(v.shape) == (self.B,) or tuple(v.shape) == (1,)):
                    raise ValueError("fixed[%r]: a scalar or a tensor of shape (%d,)" % (k, self.B))
                out[..., self.model.parameter_names.index(k)] = v.reshape(()) if (v.ndim == 1 and not per) else v
            return out.contiguous(), per
        return fixed_values(self.model.parameter_names, self._fixed, self.B)

    def _reduce(self, alpha):
        """full-order user input -> the handle's (B, q_free)"""
        a = self._as_array(alpha)
        if a.ndim == 1 or (a.ndim == 2 and int(a.shape[0]) == 1 and self.B != 1):
            a = a.reshape(1, -1).expand(self.B, -1) if _is_torch(a) else np.broadcast_to(a.reshape(1, -1), (self.B, a.size))
        if a.ndim != 2 or tuple(a.shape) != (self.B, self.q_full):
            raise ValueError("parameters are in the model's full order: shape (%d,) or (%d, %d)" % (self.q_full, self.B, self.q_full))
        if not len(self.held):
            return a if _is_torch(a) else np.ascontiguousarray(a)
        return reduce_columns(a, getattr(self, "_free_ix", self.free))

    def _expand(self, a_free):
        if not len(self.held):
            return a_free
        return expand_columns(a_free, getattr(self, "_free_ix", self.free), getattr(self, "_held_ix", self.held), self._fix_values,
                              self.q_full)

    @_device_entry
    def set_fixed(self, **values):
        """replace the values of fixed parameters (vp_set_fixed_values): ``set_fixed(tau2=3.0)``; a name that is not fixed
        raises (the mask is part of the handle).  Cached results are invalidated."""
        not_fixed = [k for k in values if k not in self._fixed]
        if not_fixed:
            raise ValueError("set_fixed: %r not among the fixed parameters %r" % (not_fixed, list(self._fixed)))
        self._fixed.update(values)
        vals, per = self._fixed_array()
        check(self.lib.vp_set_fixed_values(self._h, self._ptr(vals), int(per)))
        self._fix_values = vals
        self._have_params = False

    def set_params(self, alpha):
        return super().set_params(self._reduce(alpha))

    def params(self):
        return self._expand(super().params())

    def evaluate(self, alpha, want_residuals=True, want_jacobian=True):
        return super().evaluate(self._reduce(alpha), want_residuals, want_jacobian)

    def basis(self, alpha, skip_invariant=False, want_phi=True, want_dphi=True, out_phi=None, out_dphi=None):
        return super().basis(self._reduce(alpha), skip_invariant, want_phi, want_dphi, out_phi, out_dphi)

    def fit(self, alpha0, solver=None, want_coefficients=True):
        a, Cm, rep = super().fit(self._reduce(alpha0), solver, want_coefficients)
        return self._expand(a), Cm, rep

    def search(self, candidates, per_problem=False):
        c = self._as_array(candidates)
        if int(c.shape[-1]) != self.q_full or c.ndim != (3 if per_problem else 2):
            raise ValueError("candidates are in the model's full order: (K, %d), or (B, K, %d) with per_problem" % (self.q_full, self.q_full))
        a, idx, cost = super().search(reduce_columns(c, getattr(self, "_free_ix", self.free)), per_problem)
        return self._expand(a), idx, cost

    def set_bounds(self, lower, upper):
        def red(b):
            if b is None:
                return None
            b = np.asarray(_to_host(b), dtype=np.float64)
            if b.shape[-1:] != (self.q_full,):
                raise ValueError("bounds are in the model's full order: shape (%d,) or (%d, %d)" % (self.q_full, self.B, self.q_full))
            return b[..., self.free]
        return super().set_bounds(red(lower), red(upper))

    def statistics(self, want_confidence_sigma=True):
        st = super().statistics(want_confidence_sigma)
        keep = np.concatenate([np.arange(self.n), self.n + self.free])
        st["cov"] = scatter_square(st["cov"], keep, self.n + self.q_full)
        st["free"] = self.free.copy()
        return st

    def global_statistics(self, want_coef_cov=True, want_confidence_sigma=False):
        st = super().global_statistics(want_coef_cov, want_confidence_sigma)
        st["cov_alpha"] = scatter_square(st["cov_alpha"], self.free, self.q_full)
        if st["coef_alpha_cov"] is not None:
            st["coef_alpha_cov"] = scatter_last(st["coef_alpha_cov"], self.free, self.q_full)
        st["free"] = self.free.copy()
        return st

    def fit_trace(self, *args, **kwargs):
        raise ValueError("fit_trace: a problem with fixed parameters is a device-column handle, which records no trace")
