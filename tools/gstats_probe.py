"""vp_global_statistics at BASELINE configs[2] (1 alpha shared by S = 16384 right-hand sides, m = 2048, triple exponential
+ offset, fp64; device tensors): wall time of the whole call with every output (Cov(alpha), chi^2, the S blocks
Cov(c_s,c_s) and Cov(c_s,alpha), the 268 MB band) and without the band, next to the global fit it describes.
Run under `rocprofv3 --kernel-trace --stats` for the per-kernel times.   usage: gstats_probe.py [S] [m] [out.json]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import varpro_amd as vp
from varpro_amd import synth

S = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
m = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
out = sys.argv[3] if len(sys.argv) > 3 else None
d = synth.mrhs_triple_exp(S=S, m=m)
rng = np.random.default_rng(1)
Y = d["Y"] + 0.5 * rng.standard_normal(d["Y"].shape)
mdl = vp.multi_exponential_model(d["x"], d["tau_guess"], offset=True)
dev = torch.device("cuda", 0)
bp = vp.BatchProblem(mdl, torch.from_numpy(Y[None]).to(dev), x=torch.from_numpy(d["x"]).to(dev))
g = torch.from_numpy(d["tau_guess"][None]).to(dev)
tf = []
for _ in range(5):
    t0 = time.perf_counter()
    a, C, rep = bp.fit(g)
    torch.cuda.synchronize()
    tf.append((time.perf_counter() - t0) * 1e3)


def timed(**kw):
    ts = []
    for _ in range(20):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = bp.global_statistics(**kw)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return r, ts


full, t_full = timed(want_coef_cov=True, want_confidence_sigma=True)
_, t_blocks = timed(want_coef_cov=True, want_confidence_sigma=False)
_, t_min = timed(want_coef_cov=False, want_confidence_sigma=False)
band_bytes = S * m * 8
res = dict(S=S, m=m, fit_ms_min=min(tf), fit_ms_median=float(np.median(tf)),
           gstats_all_outputs_ms_min=min(t_full), gstats_all_outputs_ms_median=float(np.median(t_full)),
           gstats_no_band_ms_min=min(t_blocks), gstats_cov_alpha_only_ms_min=min(t_min), band_bytes=band_bytes,
           status=int(full["status"][0]), reduced_chi2=float(full["reduced_chi2"][0]),
           sd_alpha=np.sqrt(np.diag(full["cov_alpha"][0].cpu().numpy())).tolist(), alpha=a.cpu().numpy()[0].tolist())
print(json.dumps(res))
if out:
    json.dump(res, open(out, "w"), indent=1)
