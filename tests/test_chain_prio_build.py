"""The issue-slot switches (VP_FIT2_CHAIN_PRIO in vp_fit2.hpp, VP_JAC_Q2_NOCOPY in vp_fit.hpp) build in every combination:
`make ab` (the A/B library of the headline units, varpro_amd/csrc/Makefile) for gfx950 with each switch on and off -- no GPU
needed -- and tools/isa_compare.py (the disassembly per kernel symbol next to the resources of tools/kernel_resources.py)
against the build with both off, which is the code from before the switches existed:
  * every combination compiles and links;
  * only kernels of the fit2_kernel / fit_kernel families differ -- the priority helpers sit in routines that every kernel
    family shares (house_qr, evaluate_core_const_first, jac_qrfac_scaled) and must be nothing there;
  * none of the kernels that differ has more spilled VGPRs than before."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "varpro_amd", "csrc")
COMBINATIONS = [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (1, 1)]  # (VP_FIT2_CHAIN_PRIO, VP_JAC_Q2_NOCOPY); (0, 0) is the reference
MAY_CHANGE = {"fit2_kernel", "fit_kernel"}


def _tag(c):
    return "prio%d_nocopy%d" % c


def test_every_switch_combination_builds_and_changes_only_the_fit_kernels(tmp_path):
    jobs = max(1, min(16, os.cpu_count() or 1) // len(COMBINATIONS))
    procs = {c: subprocess.Popen(["make", "-C", CSRC, "ab", "-j%d" % jobs, "TAG=" + _tag(c), "AB_BUILD=%s" % (tmp_path / _tag(c)),
                                  "AB_OUT=%s" % tmp_path, "EXTRA=-DVP_FIT2_CHAIN_PRIO=%d -DVP_JAC_Q2_NOCOPY=%d" % c],
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for c in COMBINATIONS}
    lib = {}
    for c, p in procs.items():
        log = p.communicate()[0]
        assert p.returncode == 0, "%s:\n%s" % (_tag(c), log[-3000:])
        lib[c] = str(tmp_path / ("libvarpro_hip_%s.so" % _tag(c)))
        assert os.path.getsize(lib[c]) > 0
    for c in COMBINATIONS[1:]:
        out = str(tmp_path / (_tag(c) + ".json"))
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_compare.py"), lib[COMBINATIONS[0]], lib[c], "--json", out],
                       check=True, stdout=subprocess.DEVNULL)
        d = json.load(open(out))
        print(_tag(c), "kernels", d["kernels_after"], "different", d["different_per_family"])
        assert d["only_before"] == [] and d["only_after"] == [] and d["kernels_before"] == d["kernels_after"] > 0
        assert set(d["different_per_family"]) <= MAY_CHANGE, d["different_per_family"]
        assert "fit2_kernel" in d["different_per_family"]  # (the switch reached the code it is for)
        for k in d["different_kernels"]:
            assert k["resources_after"]["vgpr_spill_count"] <= k["resources_before"]["vgpr_spill_count"], k
