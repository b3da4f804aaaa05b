"""Same machine code?  Disassembles every gfx950 kernel of two builds of the library and compares the instruction text per
(code object, kernel symbol) -- addresses and encodings stripped -- next to the resources tools/kernel_resources.py reports.
usage: python tools/isa_compare.py BEFORE.so AFTER.so [--json out.json]"""
import collections, json, os, re, subprocess, sys, tempfile, shutil
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import LLVM, code_objects, kernel_notes
RES = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
LITERAL = r", (0x[0-9a-f]+|-?\d+)$"


def kernels_of(lib):
    """({(code object index, kernel symbol): (instruction lines, resources)}, padding lines dropped); the libraries compared
    are linked from the same translation units in the same order, so the index names the same unit in both"""
    tmp, out, dropped = tempfile.mkdtemp(), {}, 0
    try:
        for n, co in enumerate(code_objects(lib, tmp)):
            res = {k["symbol"].replace(".kd", ""): [k.get(f, 0) for f in RES] for k in kernel_notes(co) if "symbol" in k}
            sym, pcrel = None, 0
            # objdump prints `...` for a run of zero bytes.  As the LAST line of a kernel it is the padding up to the next
            # symbol (layout, not this kernel's code) and is dropped and counted; anywhere else it stays and is compared.
            def drop_trailing_padding():
                nonlocal dropped
                if sym and out[(n, sym)][0] and out[(n, sym)][0][-1] == "...":
                    out[(n, sym)][0].pop()
                    dropped += 1
            for line in subprocess.run([LLVM + "/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    drop_trailing_padding()
                    sym = m.group(1) if m.group(1) in res else None
                    if sym: out[(n, sym)] = ([], res[sym])
                elif sym and line.startswith("\t"):
                    ins = line.split("//")[0].strip()
                    # s_getpc_b64, s_add_u32 <literal>, s_addc_u32 <literal>: the distance to another symbol -- it moves with
                    # the layout of the code object, not with this kernel's code.  Only that exact sequence is masked.
                    if ins.startswith("s_getpc_b64"): pcrel = 2
                    elif pcrel and re.match(r"s_add%s_u32 s\d+, s\d+" % ("" if pcrel == 2 else "c") + LITERAL, ins):
                        ins, pcrel = re.sub(LITERAL, ", <pc-relative>", ins), pcrel - 1
                    else: pcrel = 0
                    out[(n, sym)][0].append(ins)
            drop_trailing_padding()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if not out: raise SystemExit("no kernels found in " + lib)
    return out, dropped


def family(sym):
    """the kernel template's own name: the last <length><identifier> of the mangled symbol's nested name"""
    m = re.match(r"_ZN?", sym)
    if not m: return sym  # (not mangled)
    i, name = m.end(), sym
    while i < len(sym) and sym[i].isdigit():
        n = re.match(r"\d+", sym[i:]).group(0)
        name, i = sym[i + len(n):i + len(n) + int(n)], i + len(n) + int(n)
    return name


(before, pad_before), (after, pad_after) = kernels_of(sys.argv[1]), kernels_of(sys.argv[2])
different, families, diff_families = [], collections.Counter(), collections.Counter()
for k in sorted(set(before) & set(after)):
    families[family(k[1])] += 1
    if before[k][0] != after[k][0] or before[k][1] != after[k][1]:
        diff_families[family(k[1])] += 1
        different.append({"code_object": k[0], "kernel": k[1], "instructions_before": len(before[k][0]), "instructions_after": len(after[k][0]),
                          "resources_equal": before[k][1] == after[k][1], "resources_before": dict(zip(RES, before[k][1])),
                          "resources_after": dict(zip(RES, after[k][1]))})
summary = {"kernels_before": len(before), "kernels_after": len(after), "trailing_padding_lines_dropped": [pad_before, pad_after],
           "only_before": sorted(map(list, set(before) - set(after))),
           "only_after": sorted(map(list, set(after) - set(before))), "identical": len(set(before) & set(after)) - len(different),
           "different": len(different), "different_with_other_resources": sum(1 for d in different if not d["resources_equal"]),
           "kernels_per_family": dict(sorted(families.items())), "different_per_family": dict(sorted(diff_families.items())),
           "different_kernels": different}
print(json.dumps({k: v for k, v in summary.items() if k != "different_kernels"}))
for d in different: print("DIFFERENT %6d -> %6d  %s" % (d["instructions_before"], d["instructions_after"], d["kernel"][:160]))
if "--json" in sys.argv: json.dump(summary, open(sys.argv[sys.argv.index("--json") + 1], "w"), indent=1)
