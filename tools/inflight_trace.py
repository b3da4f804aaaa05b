"""How consecutive fit2_kernel launches overlap with two batches in flight: runs the schedule of tools/refit_cost_probe.py (two
handles on two streams, fits enqueued alternately) for ONE library build under rocprofv3 --kernel-trace, in a run of its own, and
summarises the timestamps of the slot kernel's dispatches: per pair of consecutive launches the distance of their starts (the
step), how far launch k+1 starts before launch k ends (the overlap) and each launch's duration.  The traced host is slower than
the untraced one: the step here is a picture of the hand-over, the step TIME comes from tools/ab_inflight.py.
usage: python tools/inflight_trace.py LIB.so OUT.json          (python tools/inflight_trace.py --child: the traced loop)"""
import csv, glob, json, os, shutil, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, STEPS = 8, 48

if sys.argv[1] == "--child":
    sys.path.insert(0, ROOT)
    import torch
    import varpro_amd as vp
    from varpro_amd import synth
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.current_stream(dev), torch.cuda.Stream(device=dev)]
    hs, gs, red = [], [], []
    for i in range(2):
        d = synth.double_exp_batch(65536, m=1024, first_problem=i * 65536, noise=1e-3)
        mdl = vp.multi_exponential_model(d["x"], d["tau_guess"][0])
        with torch.cuda.stream(streams[i]):
            hs.append(vp.BatchProblem(mdl, torch.from_numpy(d["Y"]).to(dev), x=torch.from_numpy(d["x"]).to(dev)))
        gs.append(torch.from_numpy(d["tau_guess"]).to(dev))
        red.append(torch.zeros(4, dtype=torch.float64, device=dev))
    for n in (WARM, STEPS):
        for k in range(n):
            with torch.cuda.stream(streams[k % 2]):
                hs[k % 2].fit(gs[k % 2], want_coefficients=False)
                hs[k % 2].summary_device(red[k % 2])
        torch.cuda.synchronize()
    sys.exit(0)

lib, out = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
tmp = tempfile.mkdtemp()
try:
    o = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--", sys.executable,
                        os.path.abspath(__file__), "--child"], env=dict(os.environ, VARPRO_HIP_LIBRARY=lib, PYTHONPATH=ROOT), cwd=tmp,
                       capture_output=True, text=True, timeout=420)
    if o.returncode != 0:
        print("FAILED", o.stdout[-800:], o.stderr[-800:])
        sys.exit(1)  # (nothing more is started on the device)
    rows = []
    for fn in glob.glob(tmp + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(fn)):
            if "fit2_kernel" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), int(r.get("Workgroup_Size_X", r.get("Workgroup_Size", 0)) or 0),
                             int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0)))
finally:
    shutil.rmtree(tmp, ignore_errors=True)
rows.sort()
rows = rows[-STEPS:]  # (the timed leg; the warm-up leg ends in a synchronise)
us = lambda v: round(v / 1e3, 1)
pairs = [{"step_us": us(b[0] - a[0]), "overlap_us": us(a[1] - b[0]), "duration_us": us(a[1] - a[0])} for a, b in zip(rows, rows[1:])]
med = lambda k: statistics.median(p[k] for p in pairs)
res = {"library": os.path.basename(lib), "launches": len(rows), "workgroup_size": rows[0][2], "grid_size": rows[0][3],
       "median_step_us": med("step_us"), "median_overlap_us": med("overlap_us"), "median_duration_us": med("duration_us"),
       "launches_starting_inside_the_previous_one": sum(1 for p in pairs if p["overlap_us"] > 0),
       "median_overlap_share_of_duration": round(med("overlap_us") / med("duration_us"), 4), "pairs": pairs[:12]}
json.dump(res, open(out, "w"), indent=1)
print(json.dumps({k: v for k, v in res.items() if k != "pairs"}))
