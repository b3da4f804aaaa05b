"""Speed of the device-column route (VP_BASIS_GAUSS / _LORENTZ / _LINEAR) on one MI355X.
  columns: the device's and numpy's own maximum column error against long double, in units of eps (1 + |u|) |value| (the
          cases of tests/test_gpu_peak_kinds.py::test_columns_against_long_double)
  fill  : the column kernel alone through vp_basis (peaks model n = 3, p = 4, B = 65 536, m = 512 / 1024, fp64), with
          non-temporal (the default) and with ordinary stores, bytes written per second by device events, next to basis_flat_kernel (double
          exponential, vp_basis without the constant column) at the same output volume in the same process
  fit   : BatchProblem.fit of the peaks model against the best route of an OLDER library for it -- a device-pointer external
          handle driven by a torch model with fit_with_model(check_every=4) -- the two alternating, one process per leg; and
          the new route with the active count read every 4 and 16 steps (default: 8), and with ordinary stores
usage: python tools/peak_kinds_probe.py [--old-lib libvarpro_hip_old.so] [--rounds 5] [--json out.json]"""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
B = 65536


def _data(m, dev):
    import numpy as np, torch
    from test_gpu_external import peaks_data
    x = np.linspace(0.0, 10.0, m)
    _t, _c, Y, guess = peaks_data(np.random.default_rng(5), B, x, noise=1e-2)
    return x, torch.as_tensor(Y, device=dev), torch.as_tensor(guess, device=dev)


def _dev_model(x):
    import varpro_amd as vp
    from varpro_amd import basis
    return (vp.SeparableModelBuilder(["mu1", "s1", "mu2", "g2"]).initial_parameters([3.0, 0.7, 6.4, 0.9])
            .function(["mu1", "s1"], basis.GAUSS).partial_deriv("mu1").partial_deriv("s1")
            .function(["mu2", "g2"], basis.LORENTZ).partial_deriv("mu2").partial_deriv("g2")
            .invariant_function(basis.CONST).independent_variable(x).build())


def _events_ms(fn, reps=10):
    import torch
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


def child_fill(m):
    import numpy as np, torch
    import varpro_amd as vp
    from varpro_amd import synth
    dev = torch.device("cuda", 0)
    x, Y, guess = _data(m, dev)
    bp = vp.BatchProblem(_dev_model(x), Y)
    phi, dphi = bp.basis(guess)
    nbytes = B * 7 * m * 8
    ms_by_store = {}
    for name, nt in (("ordinary", 0), ("nontemporal", 1)):
        bp.set_column_fit(8, nt)
        ms_by_store[name] = _events_ms(lambda: bp.basis(guess, out_phi=phi, out_dphi=dphi))
    ms = ms_by_store["nontemporal"]  # the library's default
    bp.close(); del phi, dphi, Y
    Bf = B * 7 // 4  # double exponential without its constant column: 4 columns per problem -> the same output volume
    d = synth.double_exp_batch(1024, m=m, noise=1e-3)
    xe = np.asarray(d["x"], dtype=np.float64).reshape(-1)[:m]
    tg = torch.as_tensor(np.tile(d["tau_guess"], (Bf // 1024, 1)), device=dev)
    bf = vp.BatchProblem(vp.multi_exponential_model(xe, d["tau_guess"][0]), torch.zeros((Bf, m), dtype=torch.float64, device=dev), x=xe)
    p2, d2 = bf.basis(tg, skip_invariant=True)
    ms_flat = _events_ms(lambda: bf.basis(tg, skip_invariant=True, out_phi=p2, out_dphi=d2))
    bf.close()
    print(json.dumps(dict(leg="fill", m=m, B=B, bytes=nbytes, cols_fill_ms=ms, cols_fill_TBps=nbytes / ms / 1e9,
                          cols_fill_ordinary_ms=ms_by_store["ordinary"], cols_fill_ordinary_TBps=nbytes / ms_by_store["ordinary"] / 1e9,
                          basis_flat_ms=ms_flat, basis_flat_TBps=Bf * 4 * m * 8 / ms_flat / 1e9,
                          ratio=(nbytes / ms) / (Bf * 4 * m * 8 / ms_flat))))


def child_fit(route, m, check_every):
    import time, numpy as np, torch
    import varpro_amd as vp
    dev = torch.device("cuda", 0)
    x, Y, guess = _data(m, dev)
    if route.startswith("new"):  # new[:look_every[:nontemporal]]
        bp = vp.BatchProblem(_dev_model(x), Y)
        opt = route.split(":")[1:]
        bp.set_column_fit(int(opt[0]) if opt else 8, int(opt[1]) if len(opt) > 1 else 1)
        run = lambda: bp.fit(guess)
    else:
        from test_gpu_external import peaks_model
        from test_gpu_extfit import torch_peaks_model
        bp = vp.BatchProblem(peaks_model(x).shape(), Y)
        mdl = torch_peaks_model(x, dev)
        run = lambda: bp.fit_with_model(mdl, guess, check_every=check_every)
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
    import test_gpu_peak_kinds as T
    from test_gpu_external import gauss, gauss_dmu, gauss_dsg, lorentz, lorentz_dga, lorentz_dmu
    out = []
    for m in (200, 1000, 10001):
        for per_problem in (False, True):
            rng = np.random.default_rng(31 + m)
            Bc = 12
            x = np.linspace(0.0, 10.0, m)
            a = T._column_parameters(rng, Bc, x)
            X = x[None, :] + rng.uniform(-0.004, 0.004, (Bc, m)) if per_problem else x
            dc = vp.BatchProblem(T.dev_peaks_model(x), np.zeros((Bc, m)), x=X)
            Phi, dPhi = dc.basis(a)
            dc.close()
            Xb = X if per_problem else np.broadcast_to(x, (Bc, m))
            refs = [T._longdouble_columns(Xb[b], a[b:b + 1]) for b in range(Bc)]
            Pl, Dl, u = (np.concatenate([r[k] for r in refs]) for k in range(3))
            mu1, s1, mu2, g2 = (a[:, k:k + 1] for k in range(4))
            Pn = np.stack([gauss(Xb, mu1, s1), lorentz(Xb, mu2, g2), np.ones_like(Xb)], 1)
            Dn = np.stack([gauss_dmu(Xb, mu1, s1), gauss_dsg(Xb, mu1, s1), lorentz_dmu(Xb, mu2, g2), lorentz_dga(Xb, mu2, g2)], 1)
            uP, uD = np.concatenate([u, 0 * u, 0 * u], 1), np.concatenate([u, u, 0 * u, 0 * u], 1)
            out.append(dict(m=m, per_problem_grid=per_problem, u_max=float(np.abs(u).max()),
                            device_max=max(T._unit_errors(Phi, Pl, uP), T._unit_errors(dPhi, Dl, uD)),
                            numpy_max=max(T._unit_errors(Pn, Pl, uP), T._unit_errors(Dn, Dl, uD))))
    print(json.dumps(dict(leg="columns", unit="eps (1 + |u|) |value|", cases=out)))


def _spawn(args, lib=None, limit=300):
    env = dict(os.environ)
    if lib:
        env["VARPRO_HIP_LIBRARY"] = lib
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args, env=env,
                       capture_output=True, text=True)
    if r.returncode != 0:  # nothing more is started on the GPU after a failure
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("leg %s failed with %d" % (args, r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    a = sys.argv[1:]
    if a and a[0] == "--child-fill":
        return child_fill(int(a[1]))
    if a and a[0] == "--child-columns":
        return child_columns()
    if a and a[0] == "--child-fit":
        return child_fit(a[1], int(a[2]), int(a[3]))
    old = a[a.index("--old-lib") + 1] if "--old-lib" in a else None
    rounds = int(a[a.index("--rounds") + 1]) if "--rounds" in a else 5
    res = dict(columns=_spawn(["--child-columns"]), fill=[], fit={})
    print(json.dumps(res["columns"]), flush=True)
    for m in (512, 1024):
        res["fill"].append(_spawn(["--child-fill", str(m)]))
        print(json.dumps(res["fill"][-1]), flush=True)
    import statistics
    for m in (512, 1024):
        legs = {"new": []}
        if old:
            legs["old"] = []
        side = {"new:4": [], "new:16": [], "new:8:0": []}  # neighbouring intervals; ordinary stores into the handle's buffers
        legs.update(side)
        for rnd in range(rounds):
            for route in legs:
                if route in side and rnd >= 3:
                    continue
                r = _spawn(["--child-fit", route, str(m), "4"], lib=os.path.abspath(old) if route == "old" else None)
                legs[route].append(r["fits_per_s"])
                print(json.dumps(r), flush=True)
        s = {k: dict(median=statistics.median(v), min=min(v), max=max(v), runs=v) for k, v in legs.items()}
        if old:
            s["ratio_new_over_old"] = s["new"]["median"] / s["old"]["median"]
        res["fit"]["m%d" % m] = s
    print(json.dumps(res))
    if "--json" in a:
        json.dump(res, open(a[a.index("--json") + 1], "w"), indent=1)


if __name__ == "__main__":
    main()
