#!/usr/bin/env python3
"""Compare the device code of HIP files in two source trees, kernel symbol by kernel symbol.

    python tools/kernel_code_diff.py PARENT_TREE THIS_TREE file.hip ...

Each file (a path relative to gpflow_amd/csrc) is cross-compiled in both trees with the Makefile's flags plus
`--offload-device-only -S -Rpass-analysis=kernel-resource-usage`.  A kernel's code is the text between its label and the end of its
function, comments stripped and the function number in local labels ignored.  One line per kernel symbol:

    identical   <kernel>   <lines>  <VGPRs/AGPRs/SGPRs/scratch/LDS/occupancy>
    reordered   <kernel>   the same line count and resources, another text
    CHANGED     <kernel>   lines or a resource number differ, parent -> tree

Exit status: 1 if any kernel is CHANGED, or exists on one side only; else 0.  It compiles and compares text; it never touches a device.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

CSRC = os.path.join("gpflow_amd", "csrc")
EXTRA = ["--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage"]
RESOURCES = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"]


def makefile_flags(tree, rel):
    """HIPCC and CXXFLAGS as the tree's Makefile sets them (ARCH substituted; the per-directory additions of conv/)."""
    text = open(os.path.join(tree, CSRC, "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M).group(1).strip()
    hipcc = os.environ.get("HIPCC", var("HIPCC"))
    flags = var("CXXFLAGS").replace("$(ARCH)", os.environ.get("ARCH", var("ARCH"))).split()
    for m in re.finditer(r"^build/(\w+)/%\.o.*:\s*CXXFLAGS\s*\+=\s*(.*)$", text, re.M):
        if rel.startswith(m.group(1) + "/"):
            flags += m.group(2).split()
    return hipcc, flags


def compile_file(tree, rel, out):
    hipcc, flags = makefile_flags(tree, rel)
    run = subprocess.run([hipcc] + flags + EXTRA + [rel, "-o", out], cwd=os.path.join(tree, CSRC), stderr=subprocess.PIPE, text=True)
    if run.returncode != 0:
        sys.exit("%s: %s does not compile\n%s" % (tree, rel, run.stderr))
    return open(out).read(), run.stderr


def kernel_bodies(asm):
    """{symbol: normalised lines} of every kernel (a symbol with an .amdhsa_kernel block)."""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    bodies, name = {}, None
    for line in asm.splitlines():
        if name is None:
            m = re.match(r"^(\S+):", line)
            if m and m.group(1) in kernels:
                name, bodies[m.group(1)] = m.group(1), []
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            name = None
            continue
        line = line.split(";")[0].strip()
        if line:
            bodies[name].append(re.sub(r"\.L([A-Za-z]+)\d+_", r".L\1_", line))
    return bodies


def kernel_resources(remarks):
    """{symbol: {resource: number}} from the compiler's kernel-resource-usage remarks."""
    res, name = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if m and name:
            res[name][m.group(1)] = m.group(2)
    return res


def demangle(names):
    tool = shutil.which("llvm-cxxfilt", path=os.pathsep.join(["/opt/rocm/llvm/bin", os.environ.get("PATH", "")])) or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), stdout=subprocess.PIPE, text=True).stdout.splitlines()
    short = lambda s: re.sub(r"^void ", "", s.replace("(anonymous namespace)::", "")).split("(")[0]
    return {n: short(o) for n, o in zip(names, out)}


def main(argv):
    if len(argv) < 4:
        sys.exit(__doc__)
    parent, tree, files = argv[1], argv[2], argv[3:]
    counts = {"identical": 0, "reordered": 0, "CHANGED": 0}
    with tempfile.TemporaryDirectory() as tmp:
        for rel in files:
            sides = []
            for k, root in enumerate((parent, tree)):
                asm, remarks = compile_file(root, rel, os.path.join(tmp, "side%d.s" % k))
                sides.append((kernel_bodies(asm), kernel_resources(remarks)))
            (pb, pr), (tb, tr) = sides
            names = demangle(sorted(set(pb) | set(tb)))
            print("%s: %d kernels" % (rel, len(names)))
            for sym in sorted(names, key=lambda s: names[s]):
                if sym not in pb or sym not in tb:
                    counts["CHANGED"] += 1
                    print("  CHANGED    %-44s only in the %s" % (names[sym], "parent" if sym in pb else "tree"))
                    continue
                nums = lambda r: "/".join(r.get(sym, {}).get(k, "?") for k in RESOURCES)
                lp, lt, rp, rt = len(pb[sym]), len(tb[sym]), nums(pr), nums(tr)
                verdict = "identical" if pb[sym] == tb[sym] and rp == rt else "reordered" if (lp, rp) == (lt, rt) else "CHANGED"
                counts[verdict] += 1
                if verdict == "identical":
                    print("  identical  %-44s %5d  %s" % (names[sym], lp, rp))
                else:
                    print("  %-9s  %-44s %5d -> %-5d  %s -> %s" % (verdict, names[sym], lp, lt, rp, rt))
    print("total: %d identical, %d reordered (same lines and resources), %d changed" % (counts["identical"], counts["reordered"], counts["CHANGED"]))
    return 1 if counts["CHANGED"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
