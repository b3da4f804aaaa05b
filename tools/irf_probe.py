"""Speed and accuracy of the IRF reconvolution kinds (VP_BASIS_EXP_DECAY_IRF / VP_BASIS_IRF) on one MI355X.
  columns: the device's and numpy's own maximum column error against the defining sums in long double, in the sensitivity
          units of the recurrence (the cases of tests/test_gpu_irf.py)
  fill  : the column launch of the four-column lifetime model (two reconvolved decays + response + constant) through vp_basis,
          B = 65 536, m = 512 / 1024, fp64, bytes written per second by device events, next to cols_fill_kernel on a
          device-column model of the same output volume (VP_BASIS_EXP_DECAY x 2 + linear + constant) -- with --old-lib that
          leg runs on the older library
  fit   : BatchProblem.fit of the lifetime model against the best route of an OLDER library for it -- a device-pointer
          external handle driven by a torch model (FFT convolution) with fit_with_model(check_every=4)
  bench : the headline bench.py on this library and on the older one, alternating
Every leg is a process of its own, the legs of a comparison alternate; medians with [min, max].
--legs selects a subset (comma-separated: columns, fill, fit, bench); an existing --json file is updated, not replaced.
usage: python tools/irf_probe.py [--old-lib libvarpro_hip_old.so] [--rounds 3] [--bench-rounds 4] [--legs fill,fit] [--json out.json]"""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
B = 65536


def _events_ms(fn, reps=10):
    import torch
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


def _lifetime(m, dev):
    """(x, irf, Y, guess) of the probe's batch: 1 024 distinct problems tiled to B"""
    import numpy as np, torch
    import irf_cases as ic
    d = ic.lifetime_data(5, 1024, m)
    rep = B // 1024
    return (d["x"], torch.as_tensor(d["irf"], device=dev), torch.as_tensor(np.tile(d["Y"], (rep, 1)), device=dev),
            torch.as_tensor(np.tile(d["guess"], (rep, 1)), device=dev))


def child_fill(which, m):
    import numpy as np, torch
    import varpro_amd as vp
    from varpro_amd import basis
    dev = torch.device("cuda", 0)
    nbytes = B * 6 * m * 8  # 4 columns of Phi + 2 of dPhi
    if which == "irf":
        import irf_cases as ic
        x, irf, Y, guess = _lifetime(m, dev)
        bp = vp.BatchProblem(ic.lifetime_model(x), Y, irf=irf)
    else:  # the pointwise column kernel at the same output volume
        x = np.linspace(0.0, 25.0, m)
        mdl = (vp.SeparableModelBuilder(["tau1", "tau2"]).function(["tau1"], basis.EXP_DECAY).partial_deriv("tau1")
               .function(["tau2"], basis.EXP_DECAY).partial_deriv("tau2").invariant_function(basis.LINEAR)
               .invariant_function(basis.CONST).independent_variable(x).initial_parameters([1.0, 4.0]).build())
        rng = np.random.default_rng(5)
        guess = torch.as_tensor(np.stack([rng.uniform(0.5, 1.5, B), rng.uniform(3, 6, B)], 1), device=dev)
        bp = vp.BatchProblem(mdl, torch.zeros((B, m), dtype=torch.float64, device=dev))
    phi, dphi = bp.basis(guess)
    ms = _events_ms(lambda: bp.basis(guess, out_phi=phi, out_dphi=dphi))
    bp.close()
    print(json.dumps(dict(leg="fill", which=which, m=m, B=B, bytes=nbytes, ms=ms, TBps=nbytes / ms / 1e9)))


def torch_lifetime_model(x, irf, dev):
    """the lifetime model as a user of the older library writes it: torch on the device, the convolutions by FFT"""
    import torch
    m = x.size
    dt = float((x[-1] - x[0]) / (m - 1))
    lag = torch.arange(m, device=dev, dtype=torch.float64)[None, :]
    fi = torch.fft.rfft(irf, 2 * m)[None, :]

    def evaluate(alpha, want):
        cols, dcols = [], []
        for k in range(2):
            tau = alpha[:, k:k + 1]
            p = torch.exp(-(lag * dt) / tau)
            cols.append(torch.fft.irfft(torch.fft.rfft(p, 2 * m) * fi, 2 * m)[:, :m])
            dcols.append(torch.fft.irfft(torch.fft.rfft(p * lag, 2 * m) * fi, 2 * m)[:, :m] * (dt / tau ** 2))
        Phi = torch.stack(cols + [irf[None, :].expand_as(cols[0]), torch.ones_like(cols[0])], 1)
        return Phi.contiguous(), torch.stack(dcols, 1).contiguous()
    return evaluate


def child_fit(route, m):
    import time, torch
    import varpro_amd as vp
    import irf_cases as ic
    dev = torch.device("cuda", 0)
    x, irf, Y, guess = _lifetime(m, dev)
    if route == "new":
        bp = vp.BatchProblem(ic.lifetime_model(x), Y, irf=irf)
        run = lambda: bp.fit(guess)
    else:
        bp = vp.BatchProblem(vp.ExternalModel(4, 2, [(0, 0), (1, 1)]), Y)
        mdl = torch_lifetime_model(x, irf, dev)
        run = lambda: bp.fit_with_model(mdl, guess, check_every=4)
    out = run(); torch.cuda.synchronize()  # warm-up fit
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); out = run(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    rep = vp.BatchProblem.report_to_numpy(out[2])
    bp.close()
    print(json.dumps(dict(leg="fit", route=route, m=m, B=B, fits_per_s=B / sorted(ts)[1], ok=float((rep["termination"] > 0).mean()),
                          mean_evals=float(rep["n_evals"].mean()))))


def child_columns():
    import numpy as np
    import varpro_amd as vp
    import irf_cases as ic
    import test_gpu_irf as T
    out = []
    for dtype, ms in ((np.float64, (1, 2, 127, 128, 129, 257, 1030)), (np.float32, (255, 256, 257, 602))):
        eps = float(np.finfo(dtype).eps)
        for m in ms:
            for per_problem in (False, True):
                X, irf, a, n, _T = T._column_case(m, dtype, per_problem)
                mdl = T.mixed_model(X[0], dtype) if n == 5 else T.small_model(X[0], n, dtype)
                dc = vp.BatchProblem(mdl, np.zeros((X.shape[0], m), dtype=dtype), x=X if per_problem else X[0], irf=irf)
                Phi, dPhi = dc.basis(a)
                dc.close()
                dev = ref = 0.0
                for b in range(X.shape[0]):
                    v, dt = (irf[b] if per_problem else irf), ic.grid_step(X[b])
                    for jc, pc, k in ([(0, 0, 0), (2, 3, 3)] if n == 5 else [(0, 0, 0)]):
                        F_n, _H, D_n = ic.recurrence(v, dt, a[b, k])
                        sums = ic.direct_sums(v, dt, a[b, k])
                        dev = max(dev, *ic.column_errors(Phi[b, jc], dPhi[b, pc], v, dt, a[b, k], eps, sums))
                        ref = max(ref, *ic.column_errors(F_n, D_n, v, dt, a[b, k], eps, sums))
                out.append(dict(dtype=np.dtype(dtype).name, m=m, per_problem=per_problem, device_max=dev, numpy_max=ref))
    print(json.dumps(dict(leg="columns", unit="eps (1 + l_i) |value|", cases=out)))


def _spawn(cmd, lib=None, limit=300):
    env = dict(os.environ)
    if lib:
        env["VARPRO_HIP_LIBRARY"] = lib
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + cmd, env=env, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:  # nothing more is started on the GPU after a failure
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("leg %s failed with %d" % (cmd, r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


def _stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), runs=v)


def main():
    a = sys.argv[1:]
    me = os.path.abspath(__file__)
    if a and a[0] == "--child-fill":
        return child_fill(a[1], int(a[2]))
    if a and a[0] == "--child-columns":
        return child_columns()
    if a and a[0] == "--child-fit":
        return child_fit(a[1], int(a[2]))
    old = os.path.abspath(a[a.index("--old-lib") + 1]) if "--old-lib" in a else None
    rounds = int(a[a.index("--rounds") + 1]) if "--rounds" in a else 3
    bench_rounds = int(a[a.index("--bench-rounds") + 1]) if "--bench-rounds" in a else 4
    want = a[a.index("--legs") + 1].split(",") if "--legs" in a else ["columns", "fill", "fit", "bench"]
    out_path = a[a.index("--json") + 1] if "--json" in a else None
    res = json.load(open(out_path)) if out_path and os.path.exists(out_path) else {}
    if "columns" in want:
        res["columns"] = _spawn([me, "--child-columns"])
        print(json.dumps(res["columns"]), flush=True)
    for m in (512, 1024) if "fill" in want else ():
        legs = {"irf": [], "cols": []}
        for _ in range(rounds):
            for which in legs:
                r = _spawn([me, "--child-fill", which, str(m)], lib=old if which == "cols" else None)
                legs[which].append(r["TBps"])
                print(json.dumps(r), flush=True)
        s = {k: _stats(v) for k, v in legs.items()}
        s["ratio_irf_over_cols"] = s["irf"]["median"] / s["cols"]["median"]
        res.setdefault("fill", {})["m%d" % m] = s
    for m in (512, 1024) if "fit" in want else ():
        legs = {"new": [], "old": []}
        for _ in range(rounds):
            for route in legs:
                r = _spawn([me, "--child-fit", route, str(m)], lib=old if route == "old" else None, limit=600)
                legs[route].append(r["fits_per_s"])
                print(json.dumps(r), flush=True)
        s = {k: _stats(v) for k, v in legs.items()}
        s["ratio_new_over_old"] = s["new"]["median"] / s["old"]["median"]
        res.setdefault("fit", {})["m%d" % m] = s
    if old and bench_rounds > 0 and "bench" in want:
        legs = {"old": [], "new": []}
        for _ in range(bench_rounds):
            for which in legs:
                r = _spawn([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "50", "--warmup", "5", "--no-cpu-baseline",
                            "--no-side-configs"], lib=old if which == "old" else None, limit=600)
                legs[which].append(r["ms_per_step"])
                print(json.dumps(dict(leg="bench", which=which, ms_per_step=r["ms_per_step"])), flush=True)
        res["bench"] = {k: _stats(v) for k, v in legs.items()}
    print(json.dumps(res))
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
