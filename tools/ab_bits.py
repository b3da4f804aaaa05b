"""Bit-level comparison of library builds: fits the bench's 65 536 headline problems (and 4 096 at m = 1000, the general-length
slot kernel) with each library in its own process and prints a hash of (parameters, coefficients, reports).
--ext: the caller-evaluated family instead -- vp_evaluate_with_basis (r, J, C, cost, status) at a resident length, on four
and eight waves per problem and streamed (m = 10 000), weighted and unweighted, and one stepped fit per protocol (eager,
derivatives on accept) at a resident and a streamed length (parameters, coefficients, reports); with --time also the device
time of every leg (torch events around back-to-back calls; the fit: its first step, and end to end with the columns
recomputed by torch every step).
--cols: the device-column family (vp_cols.hpp, vp_irf.hpp) -- vp_basis of the mixed descriptor of
tests/test_gpu_cols_ordinary_stores.py (Phi, dPhi, Phi without its constant) in fp64 and fp32, in 16-byte groups and
element-wise, with shared and per-problem grids and responses, one bounded fit of that descriptor, and at the shapes of
tools/peak_kinds_probe.py, bounds_probe.py, irf_probe.py and irf_periodic_probe.py (B = 65 536, m = 512 / 1024, fp64, device
pointers) one fit each of the peaks model, the peaks model in the `wide` box, the lifetime model and the periodic lifetime
model (parameters, coefficients, reports); with --time also the device time of the column fill through vp_basis and of the fit
(the bounded kernels run inside a fit only).  The FIRST library is the reference: the JSON says whether every hash equals
its hash and where the other libraries' median times lie in its spread between rounds.
--rounds N alternates the libraries N times; --json writes every line's numbers.
usage: python tools/ab_bits.py [--ext | --cols [--time] [--rounds N] [--json out.json]] libA.so libB.so ..."""
import hashlib, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sha(*arrays):
    import numpy as np
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes())
    return h.hexdigest()[:16]


def ext_child(timed):
    import numpy as np, torch
    import varpro_amd as vp
    from varpro_amd import synth
    dev = torch.device("cuda", 0)

    def ms(fn, reps):
        fn(); torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps): fn()
            e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / reps)
        return sorted(ts)[len(ts) // 2]

    def problem(B, m, weighted):
        d = synth.double_exp_batch(B, m=m, noise=1e-3)
        x = torch.from_numpy(np.asarray(d["x"], dtype=np.float64).reshape(-1)[:m]).to(dev)
        w = (1.0 + 0.5 * torch.cos(0.01 * torch.arange(m, dtype=torch.float64, device=dev))) if weighted else None
        bp = vp.BatchProblem(vp.ExternalModel(3, 2, [(0, 0), (1, 1)]), torch.from_numpy(d["Y"]).to(dev), weights=w)

        def columns(alpha, want=None):  # exp(-x/t1), exp(-x/t2), 1 and the two derivative columns
            e = torch.exp(-x[None, None, :] / alpha[:, :, None])
            return torch.cat([e, torch.ones_like(e[:, :1])], 1).contiguous(), (e * x[None, None, :] / alpha[:, :, None] ** 2).contiguous()
        return bp, torch.from_numpy(d["tau_guess"]).to(dev), columns

    # (evaluate legs: the bench's external_model shapes; the fit legs: external_fit's)
    for name, B, m in (("resident", 65536, 1024), ("w4", 8192, 4096), ("w8", 8192, 8192), ("streamed", 4096, 10000)):
        for weighted in (False, True):
            bp, g, columns = problem(B, m, weighted)
            Phi, dPhi = columns(g)
            o = bp.evaluate_with_basis(g, Phi, dPhi)
            t = " ms %.4f" % ms(lambda: bp.evaluate_with_basis(g, Phi, dPhi), 10) if timed else ""
            print("LEG evaluate_%s_%s sha %s%s" % (name, "weighted" if weighted else "plain", sha(o["r"], o["J"], o["C"], o["cost"], o["status"]), t))
            bp.close()
            del bp, Phi, dPhi, o
    for name, B, m in (("resident", 65536, 1024), ("streamed", 4096, 10000)):
        for lazy in (False, True):
            bp, g, columns = problem(B, m, False)
            a, C, rep, steps = bp.fit_with_model(columns, g, derivatives_on_accept=lazy)
            r = bp.report_to_numpy(rep)
            t = ""
            if timed:
                Phi, dPhi = columns(g)

                def first_step():
                    bp.fit_begin(g, derivatives_on_accept=lazy)
                    bp.fit_step_with_basis(Phi, dPhi, want_count=False)
                t = " ms %.4f ms_end_to_end %.3f" % (ms(first_step, 5), ms(lambda: bp.fit_with_model(columns, g, derivatives_on_accept=lazy, check_every=4), 1))
            print("LEG fit_%s_%s sha %s evals %d steps %d%s" % (name, "on_accept" if lazy else "eager", sha(a, C, r["n_evals"], r["objective"], r["termination"]),
                                                               int(r["n_evals"].sum()), steps, t))
            bp.close()
            del bp


def cols_child(timed):
    import numpy as np, torch
    for d in ("tests", "tools"): sys.path.insert(0, os.path.join(ROOT, d))
    import varpro_amd as vp
    import irf_cases as ic, irf_periodic_cases as pc
    import test_gpu_cols_ordinary_stores as M
    import peak_kinds_probe as pk, irf_probe, irf_periodic_probe
    dev = torch.device("cuda", 0)
    for dtype in (np.float64, np.float32):
        for m in (1024, 1021):  # 16-byte groups, element-wise
            for per_problem in (False, True):
                x, irf, a = M.mixed_case(m, dtype, seed=per_problem)
                if per_problem:  # (grids shifted by multiples of 1/4: uniform and exact in fp32)
                    x = (x[None, :] + 0.25 * np.arange(M.B)[:, None]).astype(dtype)
                    irf = np.stack([ic.response(m, centre=0.05 + 0.01 * b, width=0.012) for b in range(M.B)]).astype(dtype)
                bp = vp.BatchProblem(M.mixed_model(x[0] if per_problem else x, dtype), np.zeros((M.B, m), dtype=dtype), x=x, irf=irf)
                Phi, dPhi = bp.basis(a)
                Phi_skip, _ = bp.basis(a, skip_invariant=True, want_dphi=False)
                bp.close()
                print("LEG basis_%s_m%d_%s sha %s" % (np.dtype(dtype).name, m, "per_problem" if per_problem else "shared", sha(Phi, dPhi, Phi_skip)))
    x, irf, Y, lo, hi, guess = M._fit_data()
    bp = vp.BatchProblem(M.mixed_model(x), Y, irf=irf)
    bp.set_bounds(lo, hi)
    a, C, rep = bp.fit(guess)
    bp.close()
    r = vp.BatchProblem.report_to_numpy(rep)
    print("LEG fit_mixed_bounded_m129 sha %s evals %d" % (sha(a, C, r["n_evals"], r["objective"], r["termination"]), int(r["n_evals"].sum())))

    def fit_ms(bp, guess):  # (the warm-up fit was the hashed one)
        ts = []
        for _ in range(9):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); bp.fit(guess); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return sorted(ts)[4]

    for m in (512, 1024):
        xp, Yp, gp = pk._data(m, dev)
        xl, irf_l, Yl, gl = irf_probe._lifetime(m, dev)
        mdl_p, irf_p, Yper, gper = irf_periodic_probe._data("periodic", m, dev)
        for name, make, guess in (("peaks", lambda: vp.BatchProblem(pk._dev_model(xp), Yp), gp),
                                  ("peaks_bounded", lambda: vp.BatchProblem(pk._dev_model(xp), Yp), gp),
                                  ("lifetime", lambda: vp.BatchProblem(ic.lifetime_model(xl), Yl, irf=irf_l), gl),
                                  ("lifetime_periodic", lambda: vp.BatchProblem(mdl_p, Yper, irf=irf_p), gper)):
            bp = make()
            if name == "peaks_bounded": bp.set_bounds(np.array([2.0, 0.1, 5.0, 0.1]), np.array([4.0, 2.0, 8.0, np.inf]))  # bounds_probe's `wide`
            a, C, rep = bp.fit(guess)
            r = vp.BatchProblem.report_to_numpy(rep)
            t = ""
            if timed:
                t = " ms_fit %.4f" % fit_ms(bp, guess)
                if name != "peaks_bounded":
                    phi, dphi = bp.basis(guess)
                    t += " ms_fill %.4f" % pk._events_ms(lambda: bp.basis(guess, out_phi=phi, out_dphi=dphi))
                    del phi, dphi
            print("LEG fit_%s_m%d sha %s evals %d%s" % (name, m, sha(a, C, r["n_evals"], r["objective"], r["termination"]), int(r["n_evals"].sum()), t), flush=True)
            bp.close()
            del bp


def cols_summary(record, libs):
    """every library against the first: equal hashes, and each median time within [min, max] of the first's rounds or below"""
    import statistics
    ref, legs = os.path.basename(libs[0]), sorted({r["leg"] for r in record})
    out = {"reference": ref, "hashes_equal": True, "differing_legs": [], "timing": {}}
    for leg in legs:
        if len({r["sha"] for r in record if r["leg"] == leg}) != 1:
            out["hashes_equal"] = False
            out["differing_legs"].append(leg)
        for key in ("ms_fill", "ms_fit"):
            runs = {os.path.basename(l): [r[key] for r in record if r["leg"] == leg and r["library"] == os.path.basename(l) and key in r] for l in libs}
            if not runs[ref]: continue
            e = {"reference_runs": runs[ref], "reference_median": statistics.median(runs[ref]), "reference_spread": [min(runs[ref]), max(runs[ref])]}
            for l, v in runs.items():
                if l != ref: e[l] = {"runs": v, "median": statistics.median(v), "inside_spread_or_faster": statistics.median(v) <= max(runs[ref])}
            out["timing"]["%s.%s" % (leg, key)] = e
    return out


if len(sys.argv) > 1 and sys.argv[1] == "--child":
    if "--ext" in sys.argv:
        ext_child("--time" in sys.argv)
        sys.exit(0)
    if "--cols" in sys.argv:
        cols_child("--time" in sys.argv)
        sys.exit(0)
    import numpy as np
    import varpro_amd as vp
    from varpro_amd import synth
    for B, m, fg in ((65536, 1024, None), (16384, 1000, "slots"), (4096, 1024, None)):
        d = synth.double_exp_batch(B, m=m, noise=1e-3)
        mdl = vp.multi_exponential_model(d["x"], d["tau_guess"][0])
        bp = vp.BatchProblem(mdl, d["Y"], x=d["x"])
        if fg and hasattr(bp, "set_fit_kernel"): bp.set_fit_kernel(fg)
        a, C, rep = bp.fit(d["tau_guess"])
        print("B=%d m=%d: evals %d  sha %s" % (B, m, int(rep["n_evals"].sum()), sha(a, C, rep["n_evals"], rep["objective"], rep["termination"])))
        bp.close()
    sys.exit(0)
flags = [a for a in sys.argv[1:] if a in ("--ext", "--cols", "--time")]
rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 1
record = []
for rnd in range(rounds):
    for lib in [a for a in sys.argv[1:] if a.endswith(".so")][::-1 if rnd % 2 else 1]:  # (who goes first alternates too)
        o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + flags, env=dict(os.environ, VARPRO_HIP_LIBRARY=os.path.abspath(lib), PYTHONPATH=ROOT),
                           capture_output=True, text=True, cwd=ROOT, timeout=420)
        for ln in o.stdout.splitlines():
            if ln.startswith("B=") or ln.startswith("LEG "):
                print("%-28s %s" % (os.path.basename(lib), ln), flush=True)
                w = ln.split()
                if w[0].startswith("B="):  # (plain mode) "B=65536 m=1024: evals N  sha H"
                    record.append({"library": os.path.basename(lib), "round": rnd, "B": int(w[0][2:]), "m": int(w[1][2:-1]), "evaluations": int(w[3]), "sha256_16": w[5]})
                if w[0] == "LEG": record.append(dict({"library": os.path.basename(lib), "round": rnd, "leg": w[1]},
                                   **{w[i]: (w[i + 1] if w[i] == "sha" else float(w[i + 1])) for i in range(2, len(w) - 1, 2)}))
        if o.returncode != 0:
            print(os.path.basename(lib), "FAILED", o.stderr[-600:])
            sys.exit(1)  # (nothing more is started on the device after a failed child)
if "--cols" in flags:
    summary = cols_summary(record, [a for a in sys.argv[1:] if a.endswith(".so")])
    print("SUMMARY " + json.dumps(summary))
    record = {"summary": summary, "lines": record}
if "--json" in sys.argv: json.dump(record, open(sys.argv[sys.argv.index("--json") + 1], "w"), indent=1)
