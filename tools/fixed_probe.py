"""Cost and benefit of fixed nonlinear parameters (vp_batch_create_fixed) on one MI355X, through the fit
path: B = 65 536, fp64, m = 512 / 1024, device pointers, legs
  plain    : the peaks model of tools/peak_kinds_probe.py (n = 3, p = 4) -- cols_fill_kernel, the parent's instruction text
  zero     : the same handle created with an all-zero mask -- cols_fill_fixed_kernel with the identity box: the SAME
             trajectory as `plain`, bit for bit, so the two differ by the sibling's loads, branches and multiplications alone
  widths   : both widths held at each problem's true value (p 4 -> 2)
  lt_free  : the lifetime model of tools/irf_probe.py (two reconvolved decays, response, offset; p = 2)
  lt_tau2  : tau2 held at each problem's true value (p 2 -> 1)
alternating, one process per leg and round.  Per leg: the fit rate (median of three fits), evaluations per fit, the number of
failed fits, and the time of ONE column launch over all B problems -- HIP events around vp_basis into preallocated device
arrays, median of ten -- next to the bytes that launch stores.
The column kernels' own durations come from a kernel trace of one child per leg, a run of its own
(rocprofv3 --kernel-trace --output-format csv -d DIR/LEG_M -- python tools/fixed_probe.py --child LEG M): the child ends with
11 vp_basis calls, each ONE launch of every column kernel of the leg over all B problems, so a kernel's last 10 dispatches
in time order are the timed ones; their median is the launch's time.  The dispatches before them are the 4 fits': their sum
is what the column kernels cost the fits, their 15 longest are the steps in which (nearly) all problems are still active.
usage: python tools/fixed_probe.py [--rounds 5] [--json out.json]
       python tools/fixed_probe.py --kernel-times DIR [--json out.json]"""
import csv, glob, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from peak_kinds_probe import B, _dev_model, _events_ms
LEGS = ("plain", "zero", "widths", "lt_free", "lt_tau2")


def _batch(kind, m):
    """(x, irf or None, Y, guess, truth) as numpy arrays, B problems: generated from fixed seeds by every child"""
    import numpy as np
    if kind == "peaks":
        from test_gpu_external import peaks_data
        x = np.linspace(0.0, 10.0, m)
        truth, _c, Y, guess = peaks_data(np.random.default_rng(5), B, x, noise=1e-2)
        return x, None, Y, guess, truth
    import irf_cases as ic
    d = ic.lifetime_data(5, 1024, m)  # 1 024 distinct problems tiled to B
    rep = B // 1024
    return d["x"], d["irf"], np.tile(d["Y"], (rep, 1)), np.tile(d["guess"], (rep, 1)), np.tile(d["truth"], (rep, 1))


def child(leg, m):
    import time, numpy as np, torch
    import varpro_amd as vp
    import irf_cases as ic
    dev = torch.device("cuda", 0)
    peaks = leg in ("plain", "zero", "widths")
    x, irf, Y, guess, truth = _batch("peaks" if peaks else "lifetime", m)
    t = lambda a: torch.as_tensor(a, device=dev)
    mdl = _dev_model(x) if peaks else ic.lifetime_model(x)
    kw = {} if peaks else dict(irf=t(irf))
    if leg == "zero":
        kw["fixed"] = {}
    elif leg == "widths":
        kw["fixed"] = {"s1": t(truth[:, 1].copy()), "g2": t(truth[:, 3].copy())}
    elif leg == "lt_tau2":
        kw["fixed"] = {"tau2": t(truth[:, 1].copy())}
    bp = vp.BatchProblem(mdl, t(Y), **kw)
    g = t(guess)
    run = lambda: bp.fit(g)
    out = run(); torch.cuda.synchronize()  # warm-up fit
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); out = run(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    rep = vp.BatchProblem.report_to_numpy(out[2])
    # one column launch over all B problems at the guesses: the handle's own (reduced) parameters, outputs preallocated
    a = g[:, torch.as_tensor(bp.free, device=dev)].contiguous() if "fixed" in kw else g
    phi, dphi = bp._empty((B, bp.n, m)), bp._empty((B, bp.p, m))
    col_ms = _events_ms(lambda: vp.BatchProblem.basis(bp, a, out_phi=phi, out_dphi=dphi))
    bp.close()
    fit_s = sorted(ts)[1]
    print(json.dumps(dict(leg=leg, m=m, B=B, fit_ms=1e3 * fit_s, fits_per_s=B / fit_s, failed=int((rep["termination"] <= 0).sum()),
                          mean_evals=float(rep["n_evals"].mean()), max_evals=int(rep["n_evals"].max()), col_ms=col_ms,
                          columns=int(bp.n + bp.p), col_bytes=int(B * (bp.n + bp.p) * m * 8))))


def _spawn(args, limit=300):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True)
    if r.returncode != 0:  # nothing more is started on the GPU after a failure
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("leg %s failed with %d" % (args, r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


KERNELS = ("cols_fill_fixed_kernel", "cols_fill_bounded_kernel", "cols_fill_kernel", "irf_cols_periodic_fixed_kernel",
           "irf_cols_fixed_kernel", "irf_cols_periodic_kernel", "irf_cols_kernel")


def kernel_times(top):
    """per traced leg (DIR/LEG_M) and column kernel: dispatches, the median of the last 10 in time order [us] (one vp_basis
    launch over all B), and of the 4 fits' dispatches the sum and the 15 longest [us]; per leg the sums over its kernels"""
    out = {}
    for leg_dir in sorted(d for d in glob.glob(os.path.join(top, "*")) if os.path.isdir(d)):
        per = {}
        for f in glob.glob(os.path.join(leg_dir, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                key = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
                if key:
                    per.setdefault(key, []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
        leg = {}
        for k, v in per.items():
            v = [t for _start, t in sorted(v)]
            basis, fits = v[-10:], v[:-11]
            leg[k] = dict(dispatches=len(v), basis_launches_us=[round(t, 1) for t in basis],
                          launch_over_all_B_us=round(statistics.median(basis), 1), fits_total_us=round(sum(fits), 1),
                          fits_longest15_us=[round(t, 1) for t in sorted(fits)[-15:]])
        leg["all_column_kernels"] = dict(launch_over_all_B_us=round(sum(k["launch_over_all_B_us"] for k in leg.values()), 1),
                                         fits_total_us=round(sum(k["fits_total_us"] for k in leg.values()), 1))
        out[os.path.basename(leg_dir)] = leg
    return out


def _stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), runs=v)


def main():
    a = sys.argv[1:]
    if a and a[0] == "--child":
        return child(a[1], int(a[2]))
    if a and a[0] == "--kernel-times":
        res = kernel_times(a[1])
        print(json.dumps(res))
        if "--json" in a:
            json.dump(res, open(a[a.index("--json") + 1], "w"), indent=1)
        return
    rounds = int(a[a.index("--rounds") + 1]) if "--rounds" in a else 5
    res = {}
    for m in (512, 1024):
        runs = {leg: [] for leg in LEGS}
        for _rnd in range(rounds):
            for leg in LEGS:
                runs[leg].append(_spawn(["--child", leg, str(m)]))
                print(json.dumps(runs[leg][-1]), flush=True)
        s = {}
        for leg, rs in runs.items():
            s[leg] = dict(fits_per_s=_stats([r["fits_per_s"] for r in rs]), col_ms=_stats([r["col_ms"] for r in rs]),
                          columns=rs[0]["columns"], col_bytes=rs[0]["col_bytes"], mean_evals=rs[0]["mean_evals"],
                          max_evals=rs[0]["max_evals"], failed=rs[0]["failed"])
        med = lambda leg, key: s[leg][key]["median"]
        s["spread_plain_fits"] = (s["plain"]["fits_per_s"]["max"] - s["plain"]["fits_per_s"]["min"]) / med("plain", "fits_per_s")
        s["spread_plain_col"] = (s["plain"]["col_ms"]["max"] - s["plain"]["col_ms"]["min"]) / med("plain", "col_ms")
        s["zero_over_plain_fits"] = med("zero", "fits_per_s") / med("plain", "fits_per_s")
        s["zero_over_plain_col_time"] = med("zero", "col_ms") / med("plain", "col_ms")
        for fixed_leg, free_leg in (("widths", "plain"), ("lt_tau2", "lt_free")):
            s["%s_over_%s" % (fixed_leg, free_leg)] = dict(
                fits=med(fixed_leg, "fits_per_s") / med(free_leg, "fits_per_s"),
                col_time=med(fixed_leg, "col_ms") / med(free_leg, "col_ms"),
                col_bytes=s[fixed_leg]["col_bytes"] / s[free_leg]["col_bytes"])
        res["m%d" % m] = s
        if "--json" in a:  # (after every m: a run that is cut short keeps what it has)
            json.dump(res, open(a[a.index("--json") + 1], "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
