"""The slot kernel's Gram-round switch (VP_FIT2_GRAM_ROUND in vp_fit2.hpp) builds at every value: `make ab` (the A/B library of
the headline units, varpro_amd/csrc/Makefile) for gfx950 with the switch at 0, 1 and 2 -- no GPU needed -- and
tools/isa_compare.py (the disassembly per kernel symbol next to the resources of tools/kernel_resources.py) against the build at 0,
which is the code from before the switch existed:
  * every value compiles and links;
  * only kernels of the fit2_kernel family differ -- the merged round sits behind a template flag of evaluate_core_const_first
    and of jac_qrfac_scaled, routines that fit_kernel and every other kernel family share and must get unchanged;
  * none of the kernels that differ has more spilled VGPRs than at 0 (a set that would keeps the two rounds: fit2_gram_round)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "varpro_amd", "csrc")
VALUES = [0, 1, 2]  # 0 is the reference
MAY_CHANGE = {"fit2_kernel"}


def _tag(v):
    return "gram%d" % v


def test_every_switch_value_builds_and_changes_only_the_slot_kernels(tmp_path):
    jobs = max(1, min(16, os.cpu_count() or 1) // len(VALUES))
    procs = {v: subprocess.Popen(["make", "-C", CSRC, "ab", "-j%d" % jobs, "TAG=" + _tag(v), "AB_BUILD=%s" % (tmp_path / _tag(v)),
                                  "AB_OUT=%s" % tmp_path, "EXTRA=-DVP_FIT2_GRAM_ROUND=%d" % v],
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for v in VALUES}
    lib = {}
    for v, p in procs.items():
        log = p.communicate()[0]
        assert p.returncode == 0, "%s:\n%s" % (_tag(v), log[-3000:])
        lib[v] = str(tmp_path / ("libvarpro_hip_%s.so" % _tag(v)))
        assert os.path.getsize(lib[v]) > 0
    for v in VALUES[1:]:
        out = str(tmp_path / (_tag(v) + ".json"))
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_compare.py"), lib[VALUES[0]], lib[v], "--json", out],
                       check=True, stdout=subprocess.DEVNULL)
        d = json.load(open(out))
        print(_tag(v), "kernels", d["kernels_after"], "different", d["different_per_family"])
        assert d["only_before"] == [] and d["only_after"] == [] and d["kernels_before"] == d["kernels_after"] > 0
        assert set(d["different_per_family"]) <= MAY_CHANGE, d["different_per_family"]
        assert "fit2_kernel" in d["different_per_family"]  # (the switch reached the code it is for)
        for k in d["different_kernels"]:
            assert k["resources_after"]["vgpr_spill_count"] <= k["resources_before"]["vgpr_spill_count"], k
