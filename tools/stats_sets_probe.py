"""Accuracy of vp_statistics and vp_best_fit on every compiled kernel set (the table of tests/stats_cases.py) on one MI355X.
Per case: the set the handle landed on, kappa_s (condition number of the column-scaled H), the device's error against the
oracle (worst of the case's problems; scaled covariance, conf_sigma, reduced chi2, best fit), and for fp32 handles e_np32 --
the error of the numpy restatement run in fp32 on the same inputs -- with the ratio error / max(e_np32, eps32 kappa_s)
(chi2: eps32 sqrt(m)) that the tests hold under stats_cases.FP32_MARGIN.  The record behind that margin.
usage: python tools/stats_sets_probe.py [--json out.json]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import stats_cases as SC
    import varpro_amd as vp
    KEYS = ("cov", "sigma", "chi2", "cov_unit", "sigma_unit", "best_fit")
    MARGIN = dict(cov=SC.FP32_MARGIN, sigma=SC.FP32_MARGIN, chi2=SC.FP32_MARGIN, cov_unit=SC.FP32_UNIT_MARGIN,
                  sigma_unit=SC.FP32_UNIT_MARGIN, best_fit=8.0)
    rows, worst = [], {"f64": {}, "f32": {}}
    for c in SC.CASES + SC.PER_PROBLEM_CASES + SC.DOF_EDGE_CASES:
        d, refs = SC.case_data(c), SC.reference(c)
        with vp.BatchProblem(d["model"], d["Y"], x=d["x"], weights=d["w"], stream_rows=c.stream) as bp:
            kset = bp.kernel_set()
            bp.set_params(d["alpha"])
            st, bf = bp.statistics(), bp.best_fit()
        dt = "f64" if c.dtype == SC.F64 else "f32"
        row = dict(case=SC.case_id(c), named_set=SC.set_name(c.set), set=SC.set_name(kset), dtype=dt, m=c.m,
                   status=[int(s) for s in st["status"]], kappa_s=max(r["kappa_s"] for r in refs), device={}, tolerance={})
        errs = [SC.device_errors(st, bf, b, refs[b], SC.problem_inputs(d, b)[1]) for b in range(SC.B)]
        for k in KEYS:
            row["device"][k] = max(e[k] for e in errs)
            row["tolerance"][k] = min(r["tol"][k] for r in refs)
        if c.dtype == SC.F32:
            row["e_np32"] = {k: max(r["e_np32"][k] for r in refs) for k in KEYS[:-1]}
            # per problem: the device's error over the anchor of its tolerance (tolerance / margin)
            row["ratio"] = {k: max(e[k] / (r["tol"][k] / MARGIN[k]) for e, r in zip(errs, refs)) for k in KEYS}
        else:
            row["ratio"] = {k: max(e[k] / r["tol"][k] for e, r in zip(errs, refs)) for k in KEYS}
        for k, v in row["ratio"].items():
            if v > worst[dt].get(k, (0.0, None))[0]:
                worst[dt][k] = (v, row["case"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(note="ratio: fp32 -- device error / max(e_np32, eps32 kappa_s) (chi2: eps32 sqrt(m); best_fit: eps32 n), held under "
                    "FP32_MARGIN = %g (cov, sigma, chi2), FP32_UNIT_MARGIN = %g (cov_unit = Cov / chi2, sigma_unit = sigma / sqrt(chi2)) "
                    "and 8 (best_fit); fp64 -- device error / tolerance (chi2 1e-10, cov and sigma 1e-8, best_fit 1e-10)"
                    % (SC.FP32_MARGIN, SC.FP32_UNIT_MARGIN),
               largest_ratio=worst, cases=rows)
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(dict(largest_ratio=worst)))


if __name__ == "__main__":
    main()
