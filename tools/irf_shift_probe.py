"""Speed and accuracy of the shifted IRF kinds (VP_BASIS_EXP_DECAY_IRF_SHIFT / _IRF_SHIFT / _EXP_DECAY_IRF_PERIODIC_SHIFT;
DESIGN.md section 3h) on one MI355X, beside the kind-9 lifetime model on the PARENT's library (--parent lib.so; without it,
this build's: the kernels of kind 9 are instruction-identical, profiles/irf_shift_isa.json).
  columns: the device's and the numpy mirror's maximum error of g / g' against the long-double definition and of the
           reconvolved columns of kinds 12 / 14 in the recurrence's sensitivity units (the cases of tests/test_gpu_irf_shift.py)
  fill   : the column launch through vp_basis, B = 65 536, m = 512 / 1024, fp64, by device events: the shifted lifetime model
           c1 (g * exp tau1) + c2 (g * exp tau2) + c3 g + c4 (Phi 4 columns, dPhi 5, plus g and g' written and re-read)
           against the kind-9 lifetime model (Phi 4, dPhi 2).  The yardstick is the byte ratio: 9 + 2 columns written
           against 6 (1.83), and 6 per-problem column reads of g / g' where kind 9 reads one shared response
  fit    : BatchProblem.fit fits/s of both models on their own data
Every leg is a process of its own, the legs of a comparison alternate; medians with [min, max].
usage: python tools/irf_shift_probe.py [--parent lib.so] [--rounds 3] [--legs columns,fill,fit] [--json out.json]"""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
B = 65536


def _data(kind, m, dev):
    """(model, irf, Y, guess): 1 024 distinct problems tiled to B"""
    import numpy as np, torch
    import irf_cases as ic, irf_shift_cases as sh
    if kind == "shifted":
        d = sh.shifted_data(5, 1024, m, scatter=True, width=0.03 if m < 600 else 0.012)
        mdl = sh.shifted_model(d["x"], scatter=True)
    else:
        d = ic.lifetime_data(5, 1024, m)
        mdl = ic.lifetime_model(d["x"])
    rep = B // 1024
    return (mdl, torch.as_tensor(d["irf"], device=dev), torch.as_tensor(np.tile(d["Y"], (rep, 1)), device=dev),
            torch.as_tensor(np.tile(d["guess"], (rep, 1)), device=dev))


def child_fill(kind, m):
    import torch
    import varpro_amd as vp
    from irf_probe import _events_ms
    dev = torch.device("cuda", 0)
    mdl, irf, Y, guess = _data(kind, m, dev)
    bp = vp.BatchProblem(mdl, Y, irf=irf)
    phi, dphi = bp.basis(guess)
    ms = _events_ms(lambda: bp.basis(guess, out_phi=phi, out_dphi=dphi))
    bp.close()
    cols = 4 + (5 + 2 if kind == "shifted" else 2)  # Phi + dPhi (+ g and g')
    nbytes = B * cols * m * 8
    print(json.dumps(dict(leg="fill", kind=kind, m=m, B=B, columns_written=cols, bytes=nbytes, ms=ms, TBps=nbytes / ms / 1e9)))


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
    import test_gpu_irf_shift as T
    out = []
    for dtype, ms in ((np.float64, (2, 127, 128, 129, 257, 1030)), (np.float32, (255, 256, 257, 1030))):
        for m in ms:
            for per_problem in (False, True):
                dev, ref, dev_c, ref_c = T._check_columns(m, dtype, per_problem)
                out.append(dict(dtype=np.dtype(dtype).name, m=m, per_problem=per_problem, g_device_max=dev, g_numpy_max=ref,
                                columns_device_max=dev_c, columns_numpy_max=ref_c))
    print(json.dumps(dict(leg="columns", unit_g="eps (1 + |s|) sum |w_a| |tap| (/ dt for g')", unit_columns="eps (1 + l_i) |value|",
                          cases=out)))


def _spawn(cmd, limit=300, lib=None):
    env = dict(os.environ)
    if lib:
        env["VARPRO_HIP_LIBRARY"] = lib
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + cmd, capture_output=True, text=True, cwd=ROOT, env=env)
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
    parent = os.path.abspath(a[a.index("--parent") + 1]) if "--parent" in a else None
    res = json.load(open(out_path)) if out_path and os.path.exists(out_path) else {}
    res["kind9_library"] = "parent" if parent else "this build"
    if "columns" in want:
        res["columns"] = _spawn([me, "--child-columns"])
        print(json.dumps(res["columns"]), flush=True)
    for leg, child, key in (("fill", "--child-fill", "ms"), ("fit", "--child-fit", "fits_per_s")):
        for m in (512, 1024) if leg in want else ():
            legs = {"shifted": [], "kind9": []}
            for _ in range(rounds):
                for kind in legs:
                    r = _spawn([me, child, kind, str(m)], limit=600, lib=parent if kind == "kind9" else None)
                    legs[kind].append(r[key])
                    print(json.dumps(r), flush=True)
            s = {k: _stats(v) for k, v in legs.items()}
            s["ratio_shifted_over_kind9"] = s["shifted"]["median"] / s["kind9"]["median"]
            if leg == "fill":
                s["byte_ratio_written"] = 11 / 6
            res.setdefault(leg, {})["m%d" % m] = s
    print(json.dumps(res))
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
