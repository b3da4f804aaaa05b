"""Box bounds on nonlinear parameters as a smooth re-parameterisation alpha = g(u) (the maps of MINUIT / lmfit).

A bounded ``BatchProblem.fit`` runs the unchanged Levenberg-Marquardt drivers on INTERNAL parameters u; the column kernel
evaluates the model at alpha = g(u) and scales the derivative columns by dalpha/du (varpro_amd/csrc/vp_cols.hpp).  These are
the same formulas and clamps in numpy, per parameter with bounds (lo, hi); an infinite entry means "no bound on that side":

    bounds      alpha = g(u)                       dalpha/du                 u = g^-1(alpha)
    none        u                                  1                         alpha
    lo and hi   lo + (hi - lo)/2 (sin u + 1)       (hi - lo)/2 cos u         asin(2 (alpha - lo)/(hi - lo) - 1)
    lo only     lo - 1 + sqrt(u^2 + 1)             u / sqrt(u^2 + 1)         sqrt((alpha - lo + 1)^2 - 1)  [*]
    hi only     hi + 1 - sqrt(u^2 + 1)             -u / sqrt(u^2 + 1)        sqrt((hi - alpha + 1)^2 - 1)  [*]

[*] formed as sqrt(d - 1) sqrt(d + 1), which does not overflow for a guess far from the bound.
After g the value is clamped to [lo, hi] (rounding never leaves the box); g^-1 clamps its argument to the box first.
All functions broadcast: alpha / u of shape (..., q) against lo / hi of shape (q,) or (B, q).
"""
import numpy as np


def _sides(u, lo, hi):
    u = np.asarray(u, dtype=np.float64)
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), u.shape)
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float64), u.shape)
    has_lo, has_hi = np.isfinite(lo), np.isfinite(hi)
    return u, lo, hi, has_lo & has_hi, has_lo & ~has_hi, ~has_lo & has_hi


def _clamp(a, lo, hi):
    return np.where(a < lo, lo, np.where(a > hi, hi, a))  # (a NaN stays a NaN)


def _root(u):
    """sqrt(u^2 + 1); beyond 2^27 u^2 + 1 rounds to u^2, and |u| itself does not overflow (as on the device)"""
    return np.where(np.abs(u) >= 134217728.0, np.abs(u), np.sqrt(u * u + 1.0))


def from_internal(u, lo, hi):
    """alpha = g(u), clamped to [lo, hi]"""
    u, lo, hi, both, lo_only, hi_only = _sides(u, lo, hi)
    with np.errstate(invalid="ignore", over="ignore"):
        s = _root(u)
        a = np.where(both, lo + 0.5 * (hi - lo) * (np.sin(u) + 1.0), u)
        a = np.where(lo_only, (lo - 1.0) + s, a)
        a = np.where(hi_only, (hi + 1.0) - s, a)
    return _clamp(a, lo, hi)


def dalpha_du(u, lo, hi):
    """the derivative of g at u"""
    u, lo, hi, both, lo_only, hi_only = _sides(u, lo, hi)
    with np.errstate(invalid="ignore", over="ignore"):
        s = _root(u)
        d = np.where(both, 0.5 * (hi - lo) * np.cos(u), 1.0)
        d = np.where(lo_only, u / s, d)
        d = np.where(hi_only, -(u / s), d)
    return d


def to_internal(alpha, lo, hi):
    """u = g^-1(alpha); alpha is clamped to the box first"""
    a, lo, hi, both, lo_only, hi_only = _sides(alpha, lo, hi)
    a = _clamp(a, lo, hi)
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.where(both, np.arcsin(_clamp(2.0 * (a - lo) / (hi - lo) - 1.0, -1.0, 1.0)), a)
        d = np.where(lo_only, (a - lo) + 1.0, np.where(hi_only, (hi - a) + 1.0, 1.0))
        u = np.where(lo_only | hi_only, np.sqrt(d - 1.0) * np.sqrt(d + 1.0), u)
    return u


def normalize(lower, upper, B, q):
    """What ``BatchProblem.set_bounds`` passes to the library: ``(lo, hi, per_problem)`` as contiguous float64 arrays of shape
    (q,) or (B, q), or None when both sides are None (clear the bounds).  None on one side means infinite.  Raises
    ValueError for a wrong shape, a NaN or lower >= upper."""
    if lower is None and upper is None:
        return None
    shape = None
    for side in (lower, upper):
        if side is not None:
            sh = tuple(np.shape(side))
            if sh not in ((q,), (B, q)):
                raise ValueError("bounds must have shape (q,) = (%d,) or (B, q) = (%d, %d), not %r" % (q, B, q, sh))
            if shape is None or len(sh) > len(shape):
                shape = sh
    lo = np.full(shape, -np.inf) if lower is None else np.broadcast_to(np.asarray(lower, dtype=np.float64), shape)
    hi = np.full(shape, np.inf) if upper is None else np.broadcast_to(np.asarray(upper, dtype=np.float64), shape)
    if np.isnan(lo).any() or np.isnan(hi).any():
        raise ValueError("bounds must not be NaN (use -inf / +inf or None for an unbounded side)")
    if not (lo < hi).all():
        raise ValueError("every parameter needs lower < upper (fixing a parameter by lower == upper is not supported)")
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi), len(shape) == 2
