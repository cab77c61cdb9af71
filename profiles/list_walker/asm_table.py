#!/usr/bin/env python3
"""Per-kernel device assembly and resources of two source trees, as a table.

    asm_table.py PARENT_TREE THIS_TREE [WORKDIR]

Each tree (a checkout's root: include/ and mirbft_amd/csrc/ are read) is copied
in turn to WORKDIR/tree, so both compile at ONE path, and each of UNITS is
compiled there with COMPILE.  The assembly is split per kernel from its
`.globl NAME` line to its `.Lfunc_end` label; the resources are the compiler's
kernel-resource-usage remarks.  "identical" compares that text line by line
(and says so when only comment lines, which carry no code, differ).  CPU only (no GPU is touched)."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

UNITS = ("mirsha_kernels.hip", "mirsha_expect.hip", "mirsha_commit_ring.hip")
COMPILE = ("/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -cuid=ab --cuda-device-only -S "
           "{unit} -o {out} -Rpass-analysis=kernel-resource-usage")
FIELDS = ("VGPRs", "TotalSGPRs", "ScratchSize", "Occupancy", "LDS Size")


def compile_tree(tree, work):
    dst = os.path.join(work, "tree")
    shutil.rmtree(dst, ignore_errors=True)
    for sub in ("include", os.path.join("mirbft_amd", "csrc")):
        shutil.copytree(os.path.join(tree, sub), os.path.join(dst, sub))
    kernels = {}
    for unit in UNITS:
        out = os.path.join(work, "unit.s")
        r = subprocess.run(COMPILE.format(unit=unit, out=out).split(), cwd=os.path.join(dst, "mirbft_amd", "csrc"),
                           capture_output=True, text=True, check=True)
        res, cur = {}, None
        for line in r.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = res.setdefault(m.group(1), {})
                continue
            m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", line)
            if m and cur is not None:
                cur[m.group(1).strip()] = int(m.group(2))
        name, body = None, []
        for line in open(out):
            m = re.match(r"\s*\.globl\s+(\S+)", line)
            if m and name is None:
                name, body = m.group(1), []
            if name is not None:
                body.append(line)
                if line.startswith(".Lfunc_end"):
                    if name in res:  # a kernel (device functions carry no remark)
                        kernels[name] = (unit, body, res[name])
                    name = None
    # keyed by the demangled name without its parameter list: a kernel whose
    # signature changed still meets its parent
    pretty = subprocess.run(["c++filt"] + list(kernels), capture_output=True, text=True,
                            check=True).stdout.splitlines()
    return {re.sub(r"^void ", "", p.split("(")[0]): v for p, v in zip(pretty, kernels.values())}


def main():
    parent_tree, this_tree = sys.argv[1], sys.argv[2]
    work = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="asm_table_")
    os.makedirs(work, exist_ok=True)
    parent, this = compile_tree(parent_tree, work), compile_tree(this_tree, work)
    names = sorted(set(parent) | set(this), key=lambda n: ((parent.get(n) or this[n])[0], n))
    print("| unit | kernel | identical | lines | " + " | ".join(FIELDS) + " |")
    print("|---|---|---|---|" + "---|" * len(FIELDS))
    for n in names:
        p, t = parent.get(n), this.get(n)
        unit = (p or t)[0]
        if not p or not t:
            print(f"| {unit} | `{n}` | {'only parent' if p else 'only this tree'} | | |")
            continue
        code = lambda body: [l for l in body if not l.lstrip().startswith(";")]
        same = "yes" if p[1] == t[1] else "yes (comment lines differ)" if code(p[1]) == code(t[1]) else "no"
        cell = lambda a, b: f"{a}" if a == b else f"{a} -> {b}"
        cols = [cell(p[2].get(f, 0), t[2].get(f, 0)) for f in FIELDS]
        print(f"| {unit} | `{n}` | {same} | {cell(len(p[1]), len(t[1]))} | "
              + " | ".join(cols) + " |")


if __name__ == "__main__":
    main()
