"""Start-point search helpers (host side of ``vp_search`` / ``BatchProblem.search``).

``candidate_grid`` builds the (K, q) candidate array a search takes.  ``rank_candidates`` is a numpy mirror of the device's
shared route -- weight and orthonormalise each candidate's columns by Gram-Schmidt applied twice, score every problem by
the squared length of its projection -- for the CPU tier of the tests and for callers who want to look at the scores.
Nothing here runs in a fit: the ranking of a batch is the library's HIP kernels (varpro_amd/csrc/vp_search.hpp).
"""
import itertools

import numpy as np

# a direction whose remainder after orthogonalisation is <= DROP_FACTOR * eps(dtype) * |column| is dropped (zeros)
DROP_FACTOR = 64.0


def candidate_grid(*axes, keep=None):
    """The cartesian product of ``axes`` (one 1-d sequence per nonlinear parameter) as a (K, q) float64 array, first
    axis slowest.  ``keep``: an optional predicate of q scalars -- e.g. ``lambda t1, t2: t1 < t2`` for the two decay
    times of a double exponential, whose model is symmetric in them -- candidates for which it is false are left out."""
    if not axes:
        raise ValueError("candidate_grid needs at least one axis")
    axes = [np.atleast_1d(np.asarray(a, dtype=np.float64)).ravel() for a in axes]
    rows = [c for c in itertools.product(*axes) if keep is None or keep(*c)]
    return np.array(rows, dtype=np.float64).reshape(len(rows), len(axes))


def orthonormal_basis(Phi_w, dtype=np.float64):
    """(m, n) weighted columns -> (m, n) orthonormal columns in ``dtype`` by modified Gram-Schmidt applied twice; dropped
    directions are zero columns.  Returns None when a column is not finite."""
    P = np.asarray(Phi_w).astype(dtype)
    eps = np.finfo(dtype).eps
    Q = np.zeros_like(P)
    for j in range(P.shape[1]):
        v = P[:, j].copy()
        n0 = np.sqrt((v * v).sum(dtype=dtype))
        if not np.isfinite(n0):
            return None
        for _ in range(2):
            for i in range(j):
                v = v - Q[:, i] * (Q[:, i] @ v)
        n1 = np.sqrt((v * v).sum(dtype=dtype))
        if n1 > dtype(DROP_FACTOR) * eps * n0:
            Q[:, j] = v / n1
    return Q


def rank_candidates(basis, candidates, Y, weights=None, dtype=np.float64):
    """numpy mirror of the shared route.  ``basis(alpha) -> (m, n)`` unweighted columns at one candidate; candidates (K, q);
    Y (B, m) or (B, S, m); weights None or (m,).  Returns ``(index (B,) int32, scores (B, K))``: the score of a candidate is
    sum_s sum_j (q_j . y_w,s)^2 -- its cost is 1/2 (|y_w|^2 - score) -- and -inf for a candidate with a non-finite column;
    index is the argmax (lowest index among equal scores), -1 where no candidate is finite."""
    dtype = np.dtype(dtype).type
    candidates = np.asarray(candidates, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    Y3 = Y[:, None, :] if Y.ndim == 2 else Y
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    Yw = (Y3 if w is None else Y3 * w).astype(dtype)
    B, K = Y3.shape[0], candidates.shape[0]
    scores = np.full((B, K), -np.inf, dtype=dtype)
    for k in range(K):
        with np.errstate(all="ignore"):
            P = np.asarray(basis(candidates[k]), dtype=np.float64)
            Q = orthonormal_basis(P if w is None else P * w[:, None], dtype)
        if Q is None:
            continue
        proj = Yw @ Q  # (B, S, n)
        scores[:, k] = (proj * proj).sum(axis=(1, 2), dtype=dtype)
    index = np.full(B, -1, dtype=np.int32)
    for b in range(B):
        best = dtype(-np.inf)
        for k in range(K):
            if scores[b, k] > best:
                best, index[b] = scores[b, k], k
    return index, scores
