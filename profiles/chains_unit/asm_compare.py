#!/usr/bin/env python3
"""Device-code comparison of profiles/chains_unit (needs hipcc, no GPU):

    python profiles/chains_unit/asm_compare.py PARENT_TREE [WORKDIR]

PARENT_TREE is a checkout of the parent commit (e.g. `git worktree add`).
Every .hip unit of each tree's own Makefile SRCS is compiled with
  hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S
      -Rpass-analysis=kernel-resource-usage
and each assembly file is cut into its functions (from one
"-- Begin function" line to the next), with profiles/tile_forms/asm_compare.py's
normalisation: the __hip_cuid_ lines dropped, the ordinals of .LBB<n> /
func_end<n> dropped.  Kernels are then compared BY NAME ACROSS UNITS (the chain
kernels changed unit), and one row per kernel is printed: the unit on either
side, identical or not, lines, and the compiler's resource remarks (`a -> b`:
parent -> this tree).  Under the table, for every kernel that differs, the
differing lines once comment lines are left out.  The exit status is 1 when a kernel other than those
named in MAY_DIFFER differs, a kernel exists on one side only, or a kernel's
registers rose, it gained scratch or its occupancy fell.
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = ("VGPRs", "TotalSGPRs", "ScratchSize", "Occupancy")
MAY_DIFFER = ("mirsha::chains_commit_kernel", "mirsha::chains_commit_seg_kernel")


def units(tree):
    mk = open(os.path.join(tree, "mirbft_amd/csrc/Makefile")).read()
    return [u for u in re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split() if u.endswith(".hip")]


def compile_unit(tree, unit, out):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", unit, "-o",
                        out, "-Rpass-analysis=kernel-resource-usage"],
                       cwd=os.path.join(tree, "mirbft_amd/csrc"), check=True, capture_output=True, text=True)
    return r.stderr


def remarks(stderr):
    res, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return res


def functions(path):
    """name -> normalised lines of the function (instructions, .amdhsa_ descriptor, resource .set lines)."""
    lines = [ln for ln in open(path).read().split("\n") if "__hip_cuid_" not in ln]
    lines = [re.sub(r"(\bBB|\.LBB|func_end|func_begin)\d+", r"\1", ln) for ln in lines]
    lines = [re.sub(r"(?<=\S) +;", " ;", ln) for ln in lines]  # a label's comment column moves with its width
    lines = ["\t.text" if re.match(r"\s*\.section\s+\.text\.", ln) else ln for ln in lines]
    cuts = [i for i, ln in enumerate(lines) if "; -- Begin function" in ln]
    if not cuts:
        return {}
    cuts.append(next((i for i, ln in enumerate(lines) if ".AMDGPU.gpr_maximums" in ln or ln == "\t.amdgpu_metadata"),
                     len(lines)))
    out = {}
    for a, b in zip(cuts, cuts[1:]):
        out[re.search(r"Begin function (\S+)", lines[a]).group(1)] = lines[a:b]
    return out


def tree_kernels(tree, work):
    """mangled kernel name -> (unit, lines, resources) over every unit of the tree."""
    os.makedirs(work, exist_ok=True)
    us = units(tree)
    with ThreadPoolExecutor(8) as ex:
        errs = list(ex.map(lambda u: compile_unit(tree, u, os.path.join(work, u[:-4] + ".s")), us))
    kernels = {}
    for u, err in zip(us, errs):
        res = remarks(err)
        for name, body in functions(os.path.join(work, u[:-4] + ".s")).items():
            if name in res:  # a kernel (device functions carry no remark)
                assert name not in kernels, f"{name} in two units"
                kernels[name] = (u, body, res[name])
    return kernels


def main():
    parent_tree = os.path.abspath(sys.argv[1])
    work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="chains_unit_")
    parent = tree_kernels(parent_tree, os.path.join(work, "parent"))
    this = tree_kernels(HERE, os.path.join(work, "this"))
    names = sorted(set(parent) | set(this))
    pretty = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()
    pretty = [re.sub(r"^void ", "", p.split("(")[0]) for p in pretty]
    status, others, differ = 0, 0, []
    print("| kernel | unit | identical | lines | " + " | ".join(FIELDS) + " |")
    print("|---|---|---|---|" + "---|" * len(FIELDS))
    cell = lambda a, b: f"{a}" if a == b else f"{a} -> {b}"
    code = lambda body: [ln for ln in body if not ln.lstrip().startswith(";")]
    for n, pn in sorted(zip(names, pretty), key=lambda x: x[1]):
        p, t = parent.get(n), this.get(n)
        if not p or not t:
            status = 1
            print(f"| `{pn}` | {(p or t)[0]} | {'only parent' if p else 'only this tree'} | | | | | |")
            continue
        same = p[1] == t[1]
        worse = (t[2].get("VGPRs", 0) > p[2].get("VGPRs", 0) or t[2].get("TotalSGPRs", 0) > p[2].get("TotalSGPRs", 0)
                 or t[2].get("ScratchSize", 0) > p[2].get("ScratchSize", 0)
                 or t[2].get("Occupancy", 0) < p[2].get("Occupancy", 0))
        if worse or (not same and pn not in MAY_DIFFER):
            status = 1
        if not same:
            differ.append((pn, code(p[1]), code(t[1])))
        if same and not worse and not pn.startswith("mirsha::"):  # the library kernels of mirsha_scan.hip: one line
            others += 1
            continue
        print(f"| `{pn}` | {cell(p[0], t[0])} | {'yes' if same else 'no'} | {cell(len(p[1]), len(t[1]))} | "
              + " | ".join(cell(p[2].get(f, 0), t[2].get(f, 0)) for f in FIELDS) + " |")
    print(f"\n{len(names)} kernels; {others} more (not mirsha::, the scan library's) identical in unit, text and "
          f"resources; {len(differ)} differ" + (": " + ", ".join(d[0] for d in differ) if differ else ""))
    for pn, a, b in differ:  # what differs once the comment lines (which emit nothing) are left out
        diff = list(difflib.unified_diff(a, b, "parent", "this", n=0, lineterm=""))
        print(f"\n{pn}: {len(a)} -> {len(b)} lines without comment lines, of which differ:")
        print("\n".join(diff[2:42]) if diff else "(none: comment lines only)")
    return status


if __name__ == "__main__":
    sys.exit(main())
