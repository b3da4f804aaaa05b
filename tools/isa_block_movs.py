"""Where are a kernel's register-to-register v_mov_b64 copies?  Compiles one translation unit to gfx950 assembly (no GPU needed) and
lists, per basic block of one kernel, the VALU instructions and the v_mov_b64 vreg <- vreg copies; blocks with at least --min
copies are printed.  Written for the two-column Jacobian factorisation of the slot kernel (VP_JAC_Q2_NOCOPY, vp_fit.hpp).
usage: python tools/isa_block_movs.py [--unit vp_inst_me2_f64.hip] [--kernel SYMBOL] [--min 8] [--json out.json] [-DNAME=VALUE ...]"""
import json, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "varpro_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Werror=return-type", "-Wno-unused-function", "-Wno-pass-failed",
         "-ffp-contract=on", "--cuda-device-only", "-S"]
HEADLINE = "_ZN2vp11fit2_kernelIdNS_13MultiExpModelILi2ELb1EEELi16ELi1ELi1ELi2ELi4ELi2EEEvNS_8Fit2ArgsIT_T0_EE"


def opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def blocks_of(asm, symbol):
    at = asm.index("\n%s:" % symbol)
    body = asm[at:asm.index("; Occupancy:", at)]
    out, label = [], "entry"
    cur = {"block": label, "valu": 0, "v_mov_b64_copies": 0}
    for line in body.splitlines():
        m = re.match(r"^(\.LBB\w+):|^; %(bb\.\d+):", line)
        if m:
            out.append(cur)
            cur = {"block": m.group(1) or m.group(2), "valu": 0, "v_mov_b64_copies": 0}
        elif re.match(r"^\s+v_", line):
            cur["valu"] += 1
            if re.match(r"^\s+v_mov_b64_e32 v\[\d+:\d+\], v\[\d+:\d+\]", line): cur["v_mov_b64_copies"] += 1
    out.append(cur)
    return out


defs = [a for a in sys.argv[1:] if a.startswith("-D")]
unit, kernel, least = opt("--unit", "vp_inst_me2_f64.hip"), opt("--kernel", HEADLINE), int(opt("--min", "8"))
with tempfile.TemporaryDirectory() as tmp:
    s = os.path.join(tmp, "unit.s")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + defs + [unit, "-o", s], cwd=CSRC, check=True, capture_output=True)
    blocks = blocks_of(open(s).read(), kernel)
res = {"unit": unit, "kernel": kernel, "defines": defs, "valu_instructions": sum(b["valu"] for b in blocks),
       "v_mov_b64_copies": sum(b["v_mov_b64_copies"] for b in blocks), "blocks_with_copies": [b for b in blocks if b["v_mov_b64_copies"] >= least]}
print(json.dumps(res, indent=1))
if "--json" in sys.argv: json.dump(res, open(opt("--json", None), "w"), indent=1)
