#!/usr/bin/env python3
"""Device-code comparison of profiles/tile_forms (needs hipcc, no GPU):

    python profiles/tile_forms/asm_compare.py PARENT_TREE [WORKDIR]

PARENT_TREE is a checkout of the parent commit (e.g. `git worktree add`).
Every .hip unit of the Makefile's SRCS is compiled from both trees with
  hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S
and the two assembly files are compared whole after
  * dropping the __hip_cuid_ lines (a hash of the source text), and
  * writing the CU-block kernel's new mangled name on the parent's side
    (sha256_msgs_cu_kernel<0> became a plain kernel).
A unit whose files are then equal prints "identical".  mirsha_kernels.hip
cannot be: a plain kernel is emitted at its place in the source and into
.text, the parent's template instantiation at its first use and into a comdat
section of its own, and the local labels (.LBB<n>_*, .Lfunc_end<n>) carry the
function's ordinal <n>.  For a unit that is not equal the comparison is
therefore repeated with the file cut into its functions (everything from one
"-- Begin function" line to the next: instructions, .amdhsa_ descriptor,
resource .set lines) and the kernels of its metadata note, each list sorted
by name, the ordinals dropped and the two section spellings made one.  Equal
then prints "identical per function (order differs)".  Anything else prints
DIFFERS with the first differing lines, and the exit status is 1.
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
OLD = "_ZN6mirsha21sha256_msgs_cu_kernelILi0EEEvPKhmPKmPKjS6_jPh"
NEW = "_ZN6mirsha21sha256_msgs_cu_kernelEPKhmPKmPKjS5_jPh"


def units():
    mk = open(os.path.join(HERE, "mirbft_amd/csrc/Makefile")).read()
    return [u for u in re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split() if u.endswith(".hip")]


def compile_unit(tree, unit, out):
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", unit, "-o", out],
                   cwd=os.path.join(tree, "mirbft_amd/csrc"), check=True, stderr=subprocess.DEVNULL)


def load(path):
    return [ln.replace(OLD, NEW) for ln in open(path).read().split("\n") if "__hip_cuid_" not in ln]


def by_function(lines):
    """The file as a sorted list of pieces: header, functions, trailer, metadata kernels."""
    lines = [re.sub(r"(\bBB|\.LBB|func_end|func_begin)\d+", r"\1", ln) for ln in lines]
    lines = [re.sub(r"(?<=\S) +;", " ;", ln) for ln in lines]  # a label's comment column moves with its width
    lines = ["\t.text" if re.match(r"\s*\.section\s+\.text\.", ln) else ln for ln in lines]
    meta = lines.index("\t.amdgpu_metadata")
    code, note = lines[:meta], lines[meta:]
    cuts = [i for i, ln in enumerate(code) if "; -- Begin function" in ln]
    cuts.append(next(i for i, ln in enumerate(code) if ".AMDGPU.gpr_maximums" in ln))
    tail = code[cuts[-1]:]  # its .addrsig_sym lines (the two dynamic-LDS arrays) come in order of first use
    syms = iter(sorted(ln for ln in tail if ".addrsig_sym" in ln))
    tail = [next(syms) if ".addrsig_sym" in ln else ln for ln in tail]
    pieces = [code[: cuts[0]]] + sorted(code[a:b] for a, b in zip(cuts, cuts[1:])) + [tail]
    kcuts = [i for i, ln in enumerate(note) if ln.startswith("  - .")]
    kcuts.append(next(i for i, ln in enumerate(note) if i > kcuts[-1] and re.match(r"\S", ln)))
    name = lambda k: next(ln for ln in k if ".name:" in ln and ".args" not in ln and ln.startswith("    .name:"))
    pieces += [note[: kcuts[0]]] + sorted((note[a:b] for a, b in zip(kcuts, kcuts[1:])), key=name) + [note[kcuts[-1]:]]
    return [ln for p in pieces for ln in p]


def main():
    parent = os.path.abspath(sys.argv[1])
    work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp()
    jobs = []
    for side, tree in (("parent", parent), ("this", HERE)):
        os.makedirs(os.path.join(work, side), exist_ok=True)
        jobs += [(tree, u, os.path.join(work, side, u[:-4] + ".s")) for u in units()]
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(lambda j: compile_unit(*j), jobs))
    status = 0
    for u in units():
        a, b = (load(os.path.join(work, side, u[:-4] + ".s")) for side in ("parent", "this"))
        kernels = sum(1 for ln in b if ".amdhsa_kernel " in ln)
        if a == b:
            print(f"{u}: identical ({kernels} kernels)")
            continue
        a, b = by_function(a), by_function(b)
        if a == b:
            print(f"{u}: identical per function (order differs) ({kernels} kernels)")
            continue
        status = 1
        diff = [ln for ln in difflib.unified_diff(a, b, "parent", "this", n=0, lineterm="")]
        print(f"{u}: DIFFERS ({sum(1 for ln in diff if ln[:1] in '+-') - 2} lines)")
        print("\n".join(diff[:40]))
    return status


if __name__ == "__main__":
    sys.exit(main())
