"""Can the oracle fit five exponentials + offset on the few rows of the fp32 2-row set?  The record behind the noise of the four
small cases of tests/fit_cases.py (_inputs).  CPU only.
  1. the best scaled condition number kappa_s of H = [Phi, dPhi c] over random sets of five decay times on 100 / 128 rows;
  2. for the best-conditioned and for geometric spacings: how many of the 4 cases x 5 problems the oracle fits from
     fit_guess with kappa_s <= 1e4 and cond(H)^2 eps_longdouble <= 1e-10 at its minimum, at noise 1e-3;
  3. the same for the shapes me5o / me5o_wide at lower noise.
usage: python tools/fit_inputs_probe.py [--random N] [--fitted K] [--json out.json]"""
import itertools, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import stats_cases as SC
from oracle import oracle as O

NAME = "me5o_probe"


def arg(flag, default):
    return type(default)(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default


def kappa_s(taus, m, c=27.0):
    """H at the truth on the grid 0 .. m - 1 (decay times in grid steps), columns scaled to unit length"""
    t = np.arange(m, dtype=float)
    H = np.stack([np.exp(-t / a) for a in taus] + [np.ones(m)] + [c * t / a ** 2 * np.exp(-t / a) for a in taus], 1)
    return float(np.linalg.cond(H / np.linalg.norm(H, axis=0)))


def small_cases(shape, noise):
    r2, gram = SC.me_set(SC.F32, 5, 1, 2), SC.me_set(SC.F32, 5, 1, 16, 4)
    return [SC.case(shape, SC.F32, 128, r2, noise=noise), SC.case(shape, SC.F32, 127, r2, uniform=False, noise=noise),
            SC.case(shape, SC.F32, 100, r2, weights="shared", noise=noise), SC.case(shape, SC.F32, 130, gram, weights="shared", noise=noise)]


def fitted(c):
    """(problems that meet the condition, the oracle's termination codes)"""
    d, g, n, codes = SC.case_data(c), SC.fit_guess(c), 0, []
    for b in range(SC.B):
        x, y, w = SC.problem_inputs(d, b)
        p = O.Problem(d["model"], x, y, w=w)
        p.set_params(g[b].astype(np.float64))
        codes.append(int(p.fit().termination))
        if codes[-1] <= 0:
            continue
        try:
            at = SC.reference_at(d["model"], x, y, w, p.params(), SC.F64)
        except np.linalg.LinAlgError:  # H singular to working precision
            continue
        n += at["stats"] is not None and at["kappa_s"] <= 1e4 and at["cond_H"] ** 2 * SC.EPS_LONGDOUBLE <= 1e-10
    return int(n), codes


def try_spacing(taus, span=100.0, noise=SC.NOISE):
    SC.SHAPES[NAME] = SC.Shape([SC._E] * 5 + [SC._C], [(j,) for j in range(5)] + [()], [float(t) for t in taus], span)
    SC.case_data.cache_clear()
    SC.fit_guess.cache_clear()
    return [fitted(c)[0] for c in small_cases(NAME, noise)]


out = {}
rng = np.random.default_rng(1)
cands = []
for _ in range(arg("--random", 100000)):
    taus = np.sort(np.exp(rng.uniform(np.log(0.2), np.log(300.0), 5)))
    cands.append((kappa_s(taus, 100), kappa_s(taus, 128), taus))
out["best_kappa_s"] = {"m100": min(c[0] for c in cands), "m128": min(c[1] for c in cands)}
print("best kappa_s over %d random sets of decay times: %.0f at 100 rows, %.0f at 128 rows" % (len(cands), *out["best_kappa_s"].values()))
cands.sort(key=lambda c: c[0] + c[1])
spacings = [np.round(c[2], 3) for c in cands[:arg("--fitted", 200)]]
spacings += [np.round([100.0 / ratio / f ** (4 - k) for k in range(5)], 4)
             for f, ratio in itertools.product(np.linspace(2.4, 4.4, 11), [1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0])]
spacings += [np.round([t0 * f ** k for k in range(5)], 4) for t0, f in itertools.product([1.0, 1.5, 2.0, 3.0], [2.5, 3.0, 3.5, 4.0])]
best = (0, None, None)
for taus in spacings:
    ns = try_spacing(taus)
    if sum(ns) > best[0]:
        best = (sum(ns), taus.tolist(), ns)
out["noise_1e-3"] = {"spacings": len(spacings), "most_fits_of_20": best[0], "decay_times": best[1], "per_case": best[2]}
print("noise 1e-3, %d spacings on 0 .. 100: at most %d of 20 fits meet the condition (%s: %s)" % (len(spacings), *best))
out["shapes"] = {}
for shape, noise in itertools.product(("me5o", "me5o_wide"), (1e-3, 3e-4, 1e-4, 3e-5, 1e-5)):
    res = [fitted(c) for c in small_cases(shape, noise)]
    out["shapes"]["%s %g" % (shape, noise)] = res
    print("%-10s noise %-6g fits that meet the condition per case %s  terminations %s" % (shape, noise, [r[0] for r in res], [r[1] for r in res]))
if "--json" in sys.argv:
    json.dump(out, open(arg("--json", ""), "w"), indent=1)
