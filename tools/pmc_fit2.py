"""SQ counters and kernel durations of the slot fit kernel for ONE library build, each in a run of its own (counters: rocprofv3 --pmc
and nothing else; durations: rocprofv3 --kernel-trace), over tools/slot_probe.py's 65 536 headline fits.  Writes the averages
per fit2_kernel launch, the same per LM evaluation, and the derived issue figures.
usage: python tools/pmc_fit2.py LIB.so OUT.json [COUNTER ...]"""
import collections, csv, glob, json, os, re, shutil, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lib, out = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
counters = sys.argv[3:] or ["SQ_INSTS_VALU", "SQ_INSTS_VMEM", "SQ_ACTIVE_INST_VALU", "SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES"]
env = dict(os.environ, VARPRO_HIP_LIBRARY=lib, PYTHONPATH=ROOT)
tmp = tempfile.mkdtemp()
res = {"library": os.path.basename(lib), "workload": "tools/slot_probe.py 65536 (fit2_kernel launches: 16 of 65 536 headline fits)"}


def rocprof(name, what):
    d = os.path.join(tmp, name)
    o = subprocess.run(["rocprofv3"] + what + ["--output-format", "csv", "-d", d, "-o", name, "--", sys.executable,
                        os.path.join(ROOT, "tools", "slot_probe.py"), "65536"], env=env, cwd=tmp, capture_output=True, text=True, timeout=420)
    if o.returncode != 0:
        print(name, "FAILED", o.stdout[-800:], o.stderr[-800:])
        sys.exit(1)  # (nothing more is started on the device)
    return d, o.stdout


try:
    d, stdout = rocprof("pmc", ["--pmc"] + counters)
    ev = [int(m.group(1)) for m in re.finditer(r"slots\s+fit min .*? evals (\d+)", stdout)]
    res["evaluations_per_launch"] = ev[0] if ev else None
    vals = collections.defaultdict(lambda: collections.defaultdict(float))
    for fn in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(fn)):
            if "fit2_kernel" in r["Kernel_Name"]:
                vals[r["Counter_Name"]][r["Dispatch_Id"]] += float(r["Counter_Value"])
    res["per_launch"] = {c: sum(v.values()) / len(v) for c, v in vals.items()}
    res["launches_counted"] = max([len(v) for v in vals.values()] or [0])
    if ev:
        res["per_evaluation"] = {c: v / ev[0] for c, v in res["per_launch"].items()}
    p = res["per_launch"]
    if "SQ_ACTIVE_INST_VALU" in p and "SQ_INSTS_VALU" in p:
        res["issue_cycles_per_valu_instruction"] = p["SQ_ACTIVE_INST_VALU"] / p["SQ_INSTS_VALU"]
    if "SQ_ACTIVE_INST_VALU" in p and "SQ_WAVE_CYCLES" in p:
        res["valu_active_over_wave_cycles"] = p["SQ_ACTIVE_INST_VALU"] / p["SQ_WAVE_CYCLES"]

    d, stdout = rocprof("kt", ["--kernel-trace"])
    dur = []
    for fn in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(fn)):
            if "fit2_kernel" in r["Kernel_Name"]:
                dur.append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    dur.sort()
    res["kernel_trace"] = {"launches": len(dur), "min_ms": dur[0] / 1e6 if dur else None, "median_ms": dur[len(dur) // 2] / 1e6 if dur else None}
finally:
    shutil.rmtree(tmp, ignore_errors=True)  # (also when a profiler run exceeds its time limit)
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res))
