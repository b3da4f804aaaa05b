"""Speed and accuracy of the periodic IRF reconvolution kind (VP_BASIS_EXP_DECAY_IRF_PERIODIC) against
kind 9 of the SAME build on one MI355X (kind 9's kernels are instruction-identical to the parent's: profiles/irf_periodic_isa.json).
  columns: the device's and the numpy mirror's maximum column error against the periodic sums in long double, in the
           sensitivity units of the recurrence (the cases of tests/test_gpu_irf_periodic.py)
  fill   : the column launch of the four-column lifetime model through vp_basis, B = 65 536, m = 512 / 1024, fp64, bytes
           written per second by device events: periodic decays (default period) against kind-9 decays, same data
  fit    : BatchProblem.fit fits/s of the periodic lifetime model on incomplete decays (window 12.5) beside the kind-9
           lifetime model on its own data (window 25, tools/irf_probe.py)
Every leg is a process of its own, the legs of a comparison alternate; medians with [min, max].
usage: python tools/irf_periodic_probe.py [--rounds 3] [--legs columns,fill,fit] [--json out.json]"""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
B = 65536


def _data(kind, m, dev):
    """(model, irf, Y, guess): 1 024 distinct problems tiled to B"""
    import numpy as np, torch
    import irf_cases as ic, irf_periodic_cases as pc
    d = pc.periodic_lifetime_data(5, 1024, m) if kind == "periodic" else ic.lifetime_data(5, 1024, m)
    mdl = pc.periodic_lifetime_model(d["x"]) if kind == "periodic" else ic.lifetime_model(d["x"])
    rep = B // 1024
    return (mdl, torch.as_tensor(d["irf"], device=dev), torch.as_tensor(np.tile(d["Y"], (rep, 1)), device=dev),
            torch.as_tensor(np.tile(d["guess"], (rep, 1)), device=dev))


def child_fill(kind, m):
    import torch
    import varpro_amd as vp
    import irf_cases as ic
    from irf_probe import _events_ms
    dev = torch.device("cuda", 0)
    mdl, irf, Y, guess = _data("periodic", m, dev)  # the same grid, response and parameters for both kinds
    if kind != "periodic":
        mdl = ic.lifetime_model(mdl.x)
    bp = vp.BatchProblem(mdl, Y, irf=irf)
    phi, dphi = bp.basis(guess)
    ms = _events_ms(lambda: bp.basis(guess, out_phi=phi, out_dphi=dphi))
    bp.close()
    nbytes = B * 6 * m * 8  # 4 columns of Phi + 2 of dPhi
    print(json.dumps(dict(leg="fill", kind=kind, m=m, B=B, bytes=nbytes, ms=ms, TBps=nbytes / ms / 1e9)))


def child_fit(kind, m):
    import time, torch
    import varpro_amd as vp
    dev = torch.device("cuda", 0)
    mdl, irf, Y, guess = _data(kind, m, dev)
    bp = vp.BatchProblem(mdl, Y, irf=irf)
    out = bp.fit(guess); torch.cuda.synchronize()  # warm-up fit
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); out = bp.fit(guess); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    rep = vp.BatchProblem.report_to_numpy(out[2])
    bp.close()
    print(json.dumps(dict(leg="fit", kind=kind, m=m, B=B, fits_per_s=B / sorted(ts)[1], ok=float((rep["termination"] > 0).mean()),
                          mean_evals=float(rep["n_evals"].mean()))))


def child_columns():
    import numpy as np
    import varpro_amd as vp
    import irf_cases as ic, irf_periodic_cases as pc
    import test_gpu_irf_periodic as T
    out = []
    for dtype, ms in ((np.float64, (2, 127, 128, 129, 257, 1030)), (np.float32, (255, 256, 257, 602))):
        eps = float(np.finfo(dtype).eps)
        for m in ms:
            for per_problem in (False, True):
                for longer in (False, True):
                    X, irf, a, n, period = T._column_case(m, dtype, per_problem, longer)
                    mdl = T.mixed_model(X[0], dtype) if n == 5 else T.small_model(X[0], n, dtype)
                    dc = vp.BatchProblem(mdl, np.zeros((X.shape[0], m), dtype=dtype), x=X if per_problem else X[0], irf=irf,
                                         irf_period=period)
                    Phi, dPhi = dc.basis(a)
                    dc.close()
                    dev = ref = 0.0
                    for b in range(X.shape[0]):
                        v, dt = (irf[b] if per_problem else irf), ic.grid_step(X[b])
                        for jc, pcol, k in ([(0, 0, 0), (2, 3, 3)] if n == 5 else [(0, 0, 0)]):
                            F_n, D_n = pc.mirror(v, dt, a[b, k], period)
                            sums = pc.periodic_sums(v, dt, a[b, k], period)
                            dev = max(dev, *pc.column_errors(Phi[b, jc], dPhi[b, pcol], v, dt, a[b, k], eps, sums=sums))
                            ref = max(ref, *pc.column_errors(F_n, D_n, v, dt, a[b, k], eps, sums=sums))
                    out.append(dict(dtype=np.dtype(dtype).name, m=m, per_problem=per_problem, longer_period=longer, device_max=dev,
                                    numpy_max=ref))
    print(json.dumps(dict(leg="columns", unit="eps (1 + l_i) |value|", cases=out)))


def _spawn(cmd, limit=300):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + cmd, capture_output=True, text=True, cwd=ROOT)
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
    if a and a[0] == "--child-fit":
        return child_fit(a[1], int(a[2]))
    if a and a[0] == "--child-columns":
        return child_columns()
    rounds = int(a[a.index("--rounds") + 1]) if "--rounds" in a else 3
    want = a[a.index("--legs") + 1].split(",") if "--legs" in a else ["columns", "fill", "fit"]
    out_path = a[a.index("--json") + 1] if "--json" in a else None
    res = json.load(open(out_path)) if out_path and os.path.exists(out_path) else {}
    if "columns" in want:
        res["columns"] = _spawn([me, "--child-columns"])
        print(json.dumps(res["columns"]), flush=True)
    for leg, child, key in (("fill", "--child-fill", "TBps"), ("fit", "--child-fit", "fits_per_s")):
        for m in (512, 1024) if leg in want else ():
            legs = {"periodic": [], "kind9": []}
            for _ in range(rounds):
                for kind in legs:
                    r = _spawn([me, child, kind, str(m)], limit=600)
                    legs[kind].append(r[key])
                    print(json.dumps(r), flush=True)
            s = {k: _stats(v) for k, v in legs.items()}
            s["ratio_periodic_over_kind9"] = s["periodic"]["median"] / s["kind9"]["median"]
            res.setdefault(leg, {})["m%d" % m] = s
    print(json.dumps(res))
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
