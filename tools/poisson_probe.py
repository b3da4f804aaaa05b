"""Cost and benefit of the Poisson re-weighting (vp_poisson_reweight, BatchProblem.fit_poisson).
  reweight : the re-weighting call on one MI355X, B = 65 536, m = 512 / 1024, fp64, both modes, by device events, as bytes
             moved per second beside a device-to-device copy that moves the same number of bytes, legs alternating in one
             process.  Neyman: Y read, w and Y_w written (3 arrays).  Model: the call is the best-fit launch and the
             re-weighting launch -- F written, then Y and F read, w and Y_w written (5 arrays)
  fit      : fit_poisson on the lifetime model (rounds + 1 fits, rounds + 2 re-weightings, one evaluation) beside
             rounds + 1 plain weighted fits on the same handle from the same starts; each leg a process of its own, alternating
  stat     : CPU only (the numpy mirror and the oracle, reproducible without a GPU): bias and RMS error of tau2 and of the
             offset of the double exponential for unweighted, Neyman-weighted and iterated fits at peak counts 30, 100, 300
Medians with [min, max].
usage: python tools/poisson_probe.py [--rounds 3] [--legs reweight,fit,stat] [--json out.json]"""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
B = 65536


def _tiled(wl, dev):
    import numpy as np, torch
    rep = B // wl.Y.shape[0]
    return torch.as_tensor(np.tile(wl.Y, (rep, 1)), device=dev), torch.as_tensor(np.tile(wl.guess, (rep, 1)), device=dev)


def _stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def child_reweight(m, reps=15):
    import torch
    import poisson_cases as pc
    import varpro_amd as vp
    dev = torch.device("cuda", 0)
    wl = pc.double_exp(5, 1024, m)
    Y, guess = _tiled(wl, dev)
    bp = vp.BatchProblem(wl.model(), Y, weights="neyman")
    bp.evaluate(guess, want_residuals=False, want_jacobian=False)
    bp.poisson_reweight(Y, "model")  # (allocates the best-fit buffer)
    nbytes = {"neyman": 3 * B * m * 8, "model": 5 * B * m * 8}
    src = {k: torch.empty(v // 2, dtype=torch.uint8, device=dev) for k, v in nbytes.items()}
    dst = {k: torch.empty_like(v) for k, v in src.items()}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ms = {"neyman": [], "model": [], "copy_neyman": [], "copy_model": []}
    for it in range(reps + 2):
        keep = it >= 2  # two warm-up passes over every leg
        for mode in ("neyman", "model"):
            bp.evaluate(guess, want_residuals=False, want_jacobian=False)  # (model mode needs the evaluation back)
            torch.cuda.synchronize()
            t = timed(lambda: bp.poisson_reweight(Y, mode))
            c = timed(lambda: dst[mode].copy_(src[mode]))
            if keep:
                ms[mode].append(t)
                ms["copy_" + mode].append(c)
    bp.close()
    out = dict(leg="reweight", m=m, B=B, bytes=nbytes)
    for mode in ("neyman", "model"):
        out[mode] = dict(ms=_stats(ms[mode]), copy_ms=_stats(ms["copy_" + mode]),
                         TBps=nbytes[mode] / statistics.median(ms[mode]) / 1e9,
                         copy_TBps=nbytes[mode] / statistics.median(ms["copy_" + mode]) / 1e9,
                         fraction_of_copy=statistics.median(ms["copy_" + mode]) / statistics.median(ms[mode]))
    print(json.dumps(out))


def child_fit(kind, m):
    import time, torch
    import poisson_cases as pc
    import varpro_amd as vp
    from varpro_amd.batch import POISSON_ROUNDS
    dev = torch.device("cuda", 0)
    wl = pc.lifetime(5, 1024, m)
    Y, guess = _tiled(wl, dev)
    bp = vp.BatchProblem(wl.model(), Y, weights="neyman", irf=torch.as_tensor(wl.irf, device=dev))

    def poisson():
        return bp.fit_poisson(Y, guess)[2]

    def plain():  # the same number of fits at fixed (Neyman) weights, each from the previous parameters
        a, _C, rep = bp.fit(guess)
        for _ in range(POISSON_ROUNDS):
            a, _C, rep = bp.fit(a)
        return rep

    run = poisson if kind == "poisson" else plain
    run(); torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); rep = run(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    rep = vp.BatchProblem.report_to_numpy(rep)
    bp.close()
    print(json.dumps(dict(leg="fit", kind=kind, m=m, B=B, fits=POISSON_ROUNDS + 1, seconds=sorted(ts)[1],
                          ok=float((rep["termination"] > 0).mean()))))


def leg_stat(n=256):
    import numpy as np
    import poisson_cases as pc
    from varpro_amd.batch import POISSON_ROUNDS
    out = []
    for peak in (30.0, 100.0, 300.0):
        wl = pc.double_exp(1000 + int(peak), n, peak=(peak, peak))
        fits = {"unweighted": pc.oracle_round(wl, None, wl.guess), "neyman": pc.oracle_round(wl, pc.reweight_mirror(wl.Y, None)[0], wl.guess)}
        seq = pc.iterated_fit(wl, POISSON_ROUNDS)
        fits["iterated"] = (seq[-1][0], seq[-1][1], seq[-1][2])
        row = dict(peak=peak, problems=n)
        for name, f in fits.items():
            a, C, term = f[0], f[1], f[2]
            ok = term > 0
            e_tau = (a[ok, 1] - wl.truth[ok, 1]) / wl.truth[ok, 1]
            e_off = C[ok, 2] - wl.c_true[ok, 2]
            # a low-count decay can lose its long lifetime to the offset (tau2 runs away): counted, and kept out of the moments
            kept = np.abs(e_tau) <= 1.0
            row[name] = dict(ok=int(ok.sum()), runaway=int((~kept).sum()),
                             tau2_bias=float(e_tau[kept].mean()), tau2_rms=float(np.sqrt((e_tau[kept] ** 2).mean())),
                             tau2_median=float(np.median(e_tau)), offset_bias=float(e_off[kept].mean()),
                             offset_rms=float(np.sqrt((e_off[kept] ** 2).mean())), offset_median=float(np.median(e_off)))
        out.append(row)
    return dict(leg="stat", unit="tau2: relative error (fit - truth) / truth; offset: fit - truth in counts per bin (truth 0.05 .. 0.3); "
                "bias and rms over the fits with |tau2 error| <= 1, the others counted as runaway; medians over all successful fits",
                model="double exponential + offset, m = 200", rows=out)


def _spawn(cmd, limit=600):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:  # nothing more is started on the GPU after a failure
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("leg %s failed with %d" % (cmd, r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    a = sys.argv[1:]
    me = os.path.abspath(__file__)
    if a and a[0] == "--child-reweight":
        return child_reweight(int(a[1]))
    if a and a[0] == "--child-fit":
        return child_fit(a[1], int(a[2]))
    rounds = int(a[a.index("--rounds") + 1]) if "--rounds" in a else 3
    want = a[a.index("--legs") + 1].split(",") if "--legs" in a else ["reweight", "fit", "stat"]
    out_path = a[a.index("--json") + 1] if "--json" in a else None
    res = json.load(open(out_path)) if out_path and os.path.exists(out_path) else {}
    if "stat" in want:
        res["stat"] = leg_stat()
        print(json.dumps(res["stat"]), flush=True)
    for m in (512, 1024) if "reweight" in want else ():
        res.setdefault("reweight", {})["m%d" % m] = _spawn([me, "--child-reweight", str(m)])
        print(json.dumps(res["reweight"]["m%d" % m]), flush=True)
    for m in (512, 1024) if "fit" in want else ():
        legs = {"poisson": [], "plain": []}
        for _ in range(rounds):
            for kind in legs:
                r = _spawn([me, "--child-fit", kind, str(m)])
                legs[kind].append(r["seconds"])
                print(json.dumps(r), flush=True)
        s = {k: _stats(v) for k, v in legs.items()}
        s["fits"] = r["fits"]
        s["overhead_of_the_reweighting_rounds"] = s["poisson"]["median"] / s["plain"]["median"] - 1.0
        res.setdefault("fit", {})["m%d" % m] = s
    print(json.dumps(res))
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
