"""Cost of the robust re-weighting (vp_robust_reweight) on one MI355X at B = 65 536, m = 512 / 1024,
fp64 and fp32, by device events.  Four legs, each a process of its own, alternating round by round:
  mad      the re-weighting with the scale estimated per problem (the best-fit launch, then the selection kernel)
  fixed    the re-weighting with a fixed scale (the best-fit launch, then the one-pass kernel)
  poisson  vp_poisson_reweight in model mode on the same handle: the best-fit launch and a kernel that moves five arrays and
           selects nothing -- the memory-bound yardstick
  fit      one vp_fit of that batch from the guess (--fit-library: another build of the library, e.g. the parent's)
Every leg's handle holds the double exponential with 5 % of its bins spiked and Neyman base weights.  Medians with [min, max]
over the rounds of each process's own median.
usage: python tools/robust_probe.py [--rounds 3] [--fit-library lib.so] [--json out.json]"""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
B = 65536
LEGS = ("mad", "fixed", "poisson", "fit")


def child(leg, m, dtype, reps=9):
    import numpy as np, torch
    import poisson_cases as pc
    import robust_cases as rc
    import varpro_amd as vp
    dev = torch.device("cuda", 0)
    wl = rc.contaminate(pc.double_exp(5, 1024, m, peak=rc.PEAK))
    tdt = torch.float64 if dtype == "f64" else torch.float32
    tile = lambda a: torch.as_tensor(np.tile(a, (B // a.shape[0], 1)), device=dev).to(tdt)  # noqa: E731
    Y, guess, w0 = tile(wl.Y), tile(wl.guess), tile(wl.w0)
    bp = vp.BatchProblem(wl.model(np.float64 if dtype == "f64" else np.float32), Y, weights=w0)

    def prepare():  # the re-weighting needs the evaluation back; a fit starts from the base weights
        if leg == "fit":
            bp.set_weights(w0, Y)
        else:
            bp.evaluate(guess, want_residuals=False, want_jacobian=False)

    run = {"mad": lambda: bp.robust_reweight(Y, "huber", base_weights=w0),
           "fixed": lambda: bp.robust_reweight(Y, "huber", scale=1.0, base_weights=w0),
           "poisson": lambda: bp.poisson_reweight(Y, "model"),
           "fit": lambda: bp.fit(guess)}[leg]
    ms = []
    for it in range(reps + 2):  # two warm-up passes (the first allocates the best-fit buffer)
        prepare()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record(); torch.cuda.synchronize()
        if it >= 2:
            ms.append(e0.elapsed_time(e1))
    bp.close()
    print(json.dumps(dict(leg=leg, m=m, dtype=dtype, B=B, ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))))


def _spawn(cmd, env, limit=300):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + cmd, capture_output=True, text=True, cwd=ROOT, env=env)
    if r.returncode != 0:  # nothing more is started on the GPU after a failure
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("leg %s failed with %d" % (cmd, r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    a = sys.argv[1:]
    if a and a[0] == "--child":
        return child(a[1], int(a[2]), a[3])
    rounds = int(a[a.index("--rounds") + 1]) if "--rounds" in a else 3
    fit_lib = os.path.abspath(a[a.index("--fit-library") + 1]) if "--fit-library" in a else None
    out_path = a[a.index("--json") + 1] if "--json" in a else None
    res = dict(B=B, rounds=rounds, fit_library=os.path.relpath(fit_lib, ROOT) if fit_lib else "this build", cases={})
    for dtype in ("f64", "f32"):
        for m in (512, 1024):
            ms = {leg: [] for leg in LEGS}
            for _ in range(rounds):
                for leg in LEGS:
                    env = dict(os.environ, VARPRO_HIP_LIBRARY=fit_lib) if leg == "fit" and fit_lib else dict(os.environ)
                    r = _spawn([os.path.abspath(__file__), "--child", leg, str(m), dtype], env)
                    ms[leg].append(r["ms"])
                    print(json.dumps(r), flush=True)
            case = {leg: dict(median=statistics.median(v), min=min(v), max=max(v)) for leg, v in ms.items()}
            case["mad_over_fit"] = case["mad"]["median"] / case["fit"]["median"]
            case["mad_over_poisson"] = case["mad"]["median"] / case["poisson"]["median"]
            res["cases"]["%s_m%d" % (dtype, m)] = case
            if out_path:
                json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
