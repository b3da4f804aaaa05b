"""What vp_search costs and what it buys on one MI355X, at the headline shape: B = 65 536 double
exponentials + offset, m = 1024, a 16 x 16 grid of (tau1, tau2) (K = 256; and 8 x 8, K = 64), fp64 and fp32, device pointers,
hipEvents around the calls, one process per leg:
  search : BatchProblem.search(grid) -- the shared route -- and, from a further call with vp_set_timing, its four stages
           (candidate columns, orthonormalisation, ranking product, evaluation at the winners) and the ranking kernel's
           fraction of the fp64 roof 2 B S m K n / t / 78.6 TF
  loop   : the same ranking with the means a caller had before: K calls of vp_evaluate with only cost_out, then an argmin
  fits   : synth.double_exp_batch at the bench's noise level -- share of successful fits and largest evaluation count from
           the bench's common guess and from fit_from_search with the 16 x 16 grid
Per leg: 2 warm-up calls, then 7 timed ones; the median is reported (min and max next to it).
usage: python tools/search_probe.py [--json out.json] [--B 65536] [--m 1024]
       python tools/search_probe.py --child search|loop|fits DTYPE K B M"""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP64_ROOF_TF = 78.6


def grid(K):
    import numpy as np
    import varpro_amd as vp
    side = int(round(K ** 0.5))
    return vp.candidate_grid(np.linspace(0.4, 2.2, side), np.linspace(2.4, 8.5, side))


def _timed(fn, torch, warm=2, reps=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def child(leg, dtype, K, B, m):
    import ctypes as C
    import numpy as np, torch
    import varpro_amd as vp
    from varpro_amd import synth
    np_dt = np.float64 if dtype == "f64" else np.float32
    t_dt = torch.float64 if dtype == "f64" else torch.float32
    dev = torch.device("cuda", 0)
    d = synth.double_exp_batch(B, m=m, noise=1e-3)
    mdl = vp.multi_exponential_model(d["x"].astype(np_dt), [1.0, 5.0], dtype=np_dt)
    Y = torch.as_tensor(d["Y"], device=dev).to(t_dt)
    cand = torch.as_tensor(grid(K), device=dev).to(t_dt)
    bp = vp.BatchProblem(mdl, Y)
    out = dict(leg=leg, dtype=dtype, K=int(cand.shape[0]), B=B, m=m, n=3)
    if leg == "search":
        out.update(_timed(lambda: bp.search(cand), torch))
        bp.set_timing(True)
        bp.search(cand)
        st = bp.search_stage_ms()
        bp.set_timing(False)
        out["stages_ms"] = dict(columns=st[0], orthonormalize=st[1], rank=st[2], evaluate_winners=st[3])
        out["rank_fraction_of_fp64_roof"] = 2.0 * B * m * out["K"] * 3 / (st[2] * 1e-3) / (FP64_ROOF_TF * 1e12)
        _a, idx, _c = bp.search(cand)
        out["problems_without_winner"] = int((idx < 0).sum().item())
    elif leg == "loop":
        Kc = out["K"]
        alphas = cand[:, None, :].expand(Kc, B, 2).contiguous()
        costs = torch.empty((Kc, B), dtype=torch.float64, device=dev)
        def run():
            for k in range(Kc):
                vp._lib.check(bp.lib.vp_evaluate(bp._h, C.c_void_p(alphas[k].data_ptr()), None, None, None,
                                                 C.c_void_p(costs[k].data_ptr()), None))
            return costs.argmin(0)
        out.update(_timed(run, torch, warm=1, reps=3))
        # the two rankings agree wherever the loop's own costs separate the best two candidates by more than rounding
        _a, idx, _c = bp.search(cand)
        best = run()
        out["index_agreement"] = float((idx.long() == best).double().mean().item())
    elif leg == "fits":
        guess = torch.as_tensor(d["tau_guess"], device=dev).to(t_dt)
        for name, fit in (("guess", lambda: bp.fit(guess)), ("search", lambda: bp.fit_from_search(cand))):
            rep = vp.BatchProblem.report_to_numpy(fit()[2])
            out[name] = dict(ok_share=float((rep["termination"] > 0).mean()), failed=int((rep["termination"] <= 0).sum()),
                             max_evals=int(rep["n_evals"].max()), mean_evals=float(rep["n_evals"].mean()))
            out[name].update({"fit_" + k: v for k, v in _timed(fit, torch, warm=0, reps=3).items()})
    bp.close()
    print(json.dumps(out))


def _spawn(args, limit=240):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args],
                       capture_output=True, text=True)
    if r.returncode != 0:  # nothing more is started on the GPU after a failure
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("leg %s failed with %d" % (args, r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    a = sys.argv[1:]
    if a and a[0] == "--child":
        return child(a[1], a[2], int(a[3]), int(a[4]), int(a[5]))
    B = int(a[a.index("--B") + 1]) if "--B" in a else 65536
    m = int(a[a.index("--m") + 1]) if "--m" in a else 1024
    res = dict(B=B, m=m, fp64_roof_tf=FP64_ROOF_TF, legs=[])
    for dtype, K in (("f64", 256), ("f64", 64), ("f32", 256)):
        s = _spawn(["search", dtype, K, B, m])
        lp = _spawn(["loop", dtype, K, B, m])
        res["legs"] += [s, lp]
        res["%s_K%d_loop_over_search" % (dtype, K)] = lp["median_ms"] / s["median_ms"]
        print(json.dumps(res["legs"][-2]), flush=True)
        print(json.dumps(res["legs"][-1]), flush=True)
    res["fits"] = _spawn(["fits", "f64", 256, B, m])
    print(json.dumps(res["fits"]), flush=True)
    if "--json" in a:
        json.dump(res, open(a[a.index("--json") + 1], "w"), indent=1)


if __name__ == "__main__":
    main()
