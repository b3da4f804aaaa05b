"""Cost of box bounds in the column kernel (vp_set_bounds) on one MI355X, through the fit path: the
peaks model of tools/peak_kinds_probe.py (n = 3, p = 4, B = 65 536, m = 512 / 1024, fp64, device pointers), legs
  free : no bounds -- cols_fill_kernel, whose instruction text is the parent's (profiles/bounds_isa.json)
  inf  : bounds all infinite -- cols_fill_bounded_kernel with the identity map: the SAME trajectory as `free`, bit for bit,
         so the two differ by the bounded kernel's extra loads, branches and multiplications alone
  wide : lo = [2, 0.1, 5, 0.1], hi = [4, 2, 8, inf] (every guess of the data strictly inside) -- three sin/cos maps and one sqrt map per thread and basis loop; the
         fit takes another trajectory (it iterates on internal parameters), so evaluations per fit are printed next to it
alternating, one process per leg.  The column kernels' own durations come from a kernel trace of one child per leg
(rocprofv3 --kernel-trace --output-format csv -d DIR/LEG_M -- python tools/bounds_probe.py --child LEG M): every fit's FIRST
column launch covers all B problems, so the four longest dispatches of a kernel are that launch of the four fits.
usage: python tools/bounds_probe.py [--rounds 5] [--json out.json]
       python tools/bounds_probe.py --kernel-times DIR [--json out.json]"""
import csv, glob, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from peak_kinds_probe import B, _data, _dev_model


def child(leg, m):
    import time, numpy as np, torch
    import varpro_amd as vp
    dev = torch.device("cuda", 0)
    x, Y, guess = _data(m, dev)
    bp = vp.BatchProblem(_dev_model(x), Y)
    if leg == "inf":
        bp.set_bounds(np.full(4, -np.inf), np.full(4, np.inf))
    elif leg == "wide":
        lo, hi = np.array([2.0, 0.1, 5.0, 0.1]), np.array([4.0, 2.0, 8.0, np.inf])
        bp.set_bounds(lo, hi)
        g = guess.cpu().numpy()
        assert ((g > lo) & (g < hi)).all()  # (the data's guesses lie strictly inside)
    run = lambda: bp.fit(guess)
    out = run(); torch.cuda.synchronize()  # warm-up fit
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); out = run(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    rep = vp.BatchProblem.report_to_numpy(out[2])
    bp.close()
    t = sorted(ts)[1]
    print(json.dumps(dict(leg=leg, m=m, B=B, fit_ms=1e3 * t, fits_per_s=B / t, ok=float((rep["termination"] > 0).mean()),
                          mean_evals=float(rep["n_evals"].mean()), max_evals=int(rep["n_evals"].max()))))


def _spawn(args, limit=300):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True)
    if r.returncode != 0:  # nothing more is started on the GPU after a failure
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("leg %s failed with %d" % (args, r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


def kernel_times(top):
    """per traced leg (DIR/LEG_M) and column kernel: launches, the four longest dispatches and their median [us], the sum"""
    out = {}
    for leg_dir in sorted(d for d in glob.glob(os.path.join(top, "*")) if os.path.isdir(d)):
        per = {}
        for f in glob.glob(os.path.join(leg_dir, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                if "cols_fill" in r["Kernel_Name"]:
                    key = "cols_fill_bounded_kernel" if "bounded" in r["Kernel_Name"] else "cols_fill_kernel"
                    per.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        out[os.path.basename(leg_dir)] = {k: dict(launches=len(v), longest4_us=sorted(v)[-4:], total_us=round(sum(v), 1),
                                                  median_of_longest4_us=round(statistics.median(sorted(v)[-4:]), 1)) for k, v in per.items()}
    return out


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
        legs = {"free": [], "inf": [], "wide": []}
        for _rnd in range(rounds):
            for leg in legs:
                legs[leg].append(_spawn(["--child", leg, str(m)]))
                print(json.dumps(legs[leg][-1]), flush=True)
        s = {}
        for leg, runs in legs.items():
            v = [r["fits_per_s"] for r in runs]
            s[leg] = dict(median=statistics.median(v), min=min(v), max=max(v), runs=v, mean_evals=runs[0]["mean_evals"],
                          max_evals=runs[0]["max_evals"], ok=runs[0]["ok"])
        s["ratio_inf_over_free"] = s["inf"]["median"] / s["free"]["median"]
        s["ratio_wide_over_free"] = s["wide"]["median"] / s["free"]["median"]
        s["spread_free"] = (s["free"]["max"] - s["free"]["min"]) / s["free"]["median"]
        res["m%d" % m] = s
    print(json.dumps(res))
    if "--json" in a:
        json.dump(res, open(a[a.index("--json") + 1], "w"), indent=1)


if __name__ == "__main__":
    main()
