"""The slot kernel's critical-path switches (vp_fit2.hpp: VP_FIT2_SCALARS, VP_FIT2_LOCAL_CALLS, VP_FIT2_SKIP_REFILL) build
both ways: the headline translation unit is compiled for gfx950 to assembly once with all of them on and once with all off
(no GPU needed), and the headline instantiation -- fit2_kernel<double, MultiExpModel<2, true>, 16, 1, 1, 2, 4, 2> -- keeps
two waves per SIMD in both."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "varpro_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the Makefile's flags (without the bundle compression, which does not apply to assembly output)
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Werror=return-type", "-Wno-unused-function",
         "-Wno-pass-failed", "-ffp-contract=on", "--cuda-device-only", "-S"]
SWITCHES = ("VP_FIT2_SCALARS", "VP_FIT2_LOCAL_CALLS", "VP_FIT2_SKIP_REFILL")
HEADLINE = "_ZN2vp11fit2_kernelIdNS_13MultiExpModelILi2ELb1EEELi16ELi1ELi1ELi2ELi4ELi2EEEvNS_8Fit2ArgsIT_T0_EE"


def _kernel_info(asm, symbol):
    """the compiler's resource comments that follow a kernel's code: {"Occupancy": 2, "ScratchSize": ..., "NumVgprs": ...}"""
    at = asm.index("\n%s:" % symbol)
    end = asm.index("; Occupancy:", at)
    end = asm.index("\n", end)
    return {k: int(v) for k, v in re.findall(r"^; (\w+): (\d+)\s*$", asm[at:end], re.M)}


def test_headline_unit_compiles_with_the_switches_on_and_off(tmp_path):
    outs = {v: str(tmp_path / ("me2_%d.s" % v)) for v in (1, 0)}
    procs = {v: subprocess.Popen([HIPCC] + FLAGS + ["-D%s=%d" % (s, v) for s in SWITCHES] + ["vp_inst_me2_f64.hip", "-o", outs[v]],
                                 cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for v in (1, 0)}
    info = {}
    for v, p in procs.items():
        log = p.communicate()[0]
        assert p.returncode == 0, "switches = %d:\n%s" % (v, log[-3000:])
        info[v] = _kernel_info(open(outs[v]).read(), HEADLINE)
        print("switches = %d:" % v, info[v])
    for v in (1, 0):
        assert info[v]["Occupancy"] == 2, (v, info[v])
    # what the switches are for: not a byte more scratch, not a register more
    assert info[1]["ScratchSize"] <= info[0]["ScratchSize"] and info[1]["NumVgprs"] <= info[0]["NumVgprs"], info
