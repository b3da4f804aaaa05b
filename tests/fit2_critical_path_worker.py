"""Worker of tests/test_gpu_fit2_critical_path.py: the slot kernel on groups of FOUR waves -- the triple exponential + offset at
1024 < m <= 2048 rows (vp_inst_me3_f64.hip: 8 rows per lane x 4 waves, three slots per group), m = 1500 and 2048, B = 37 -- against
the one-problem-per-group kernel, in a process of its own so that the caller can bound it with a time limit: with W > 1 every wave of a group must take the refill-skip branch on the same LDS value, and a wave that
did not would wait at a workgroup barrier for ever.  Prints "OK <evaluations>" and exits 0 when both kernels agree bit for bit.
usage: python fit2_critical_path_worker.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import varpro_amd as vp  # noqa: E402
from varpro_amd import synth  # noqa: E402

ok, evals = True, 0
for m in (1500, 2048):
    B = 37
    d = synth.multi_exp_batch(B, 3, m, [1.0, 3.0, 7.0], noise=1e-3)
    mdl = vp.multi_exponential_model(d["x"], d["tau_guess"][0])
    out = {}
    for kernel in ("wave", "slots"):
        bp = vp.BatchProblem(mdl, d["Y"], x=d["x"])
        bp.set_fit_kernel(kernel)
        a, c, rep = bp.fit(d["tau_guess"])
        out[kernel] = (np.asarray(a), bp.report_to_numpy(rep))
        bp.close()
    (a0, r0), (a1, r1) = out["wave"], out["slots"]
    same = (np.array_equal(a0, a1, equal_nan=True) and np.array_equal(r0["termination"], r1["termination"])
            and np.array_equal(r0["n_evals"], r1["n_evals"]) and np.array_equal(r0["objective"], r1["objective"], equal_nan=True)
            and int(r1["n_evals"].min()) >= 1)
    print("m = %d: %s, evaluations %d" % (m, "same" if same else "MISMATCH", int(r1["n_evals"].sum())))
    ok = ok and same
    evals += int(r1["n_evals"].sum())
print("%s %d" % ("OK" if ok else "MISMATCH", evals))
sys.exit(0 if ok else 1)
