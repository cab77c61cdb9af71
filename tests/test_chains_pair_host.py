"""Host-side surface of the chains' SHA-512/256 pair route (no GPU): the entry
that shows the route, its NULL answers, the Python property, the threshold the
chains route by, and that the change which brought the route left the one-lane
chain kernels, the other SHA-512/256 units and the SHA-256 kernel sources (the
inputs of bench.py's traffic_key) byte for byte alone."""
import ctypes
import os
import re
import subprocess

import pytest

import mirbft_amd
from mirbft_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mirbft_amd", "csrc")
UNTOUCHED = ["mirbft_amd/csrc/mirsha_kernels.hip", "mirbft_amd/csrc/mirsha_kernels.h",
             "mirbft_amd/csrc/sha256_device.h", "mirbft_amd/csrc/sha256_rounds_asm.h",
             "mirbft_amd/csrc/mirsha_sha512.hip", "mirbft_amd/csrc/mirsha_sha512_plan.hip",
             "mirbft_amd/csrc/mirsha_sha512_chains.hip"]
NEW_UNIT = "mirbft_amd/csrc/mirsha_sha512_chains_pair.hip"


def test_the_entry_is_bound_with_the_headers_arity():
    with open(os.path.join(ROOT, "include", "mirsha.h")) as f:
        header = f.read()
    name, arity = "mirsha_chains_pair_launches", 2
    m = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
    assert m, name
    assert len(m.group(1).split(",")) == arity
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == arity
    assert hasattr(_lib.load(), name)
    assert isinstance(mirbft_amd.CheckpointChains.pair_launches, property)


def test_pair_launches_null_answers():
    lib = _lib.load()
    n = ctypes.c_uint64(7)
    assert lib.mirsha_chains_pair_launches(None, ctypes.byref(n)) == _lib.MIRSHA_EINVAL
    assert lib.mirsha_chains_pair_launches(None, None) == _lib.MIRSHA_EINVAL
    assert n.value == 7


def test_the_chains_route_by_the_threshold_of_the_other_pair_launches():
    """The measurement's decision rule (the largest measured
    group count at which the pair's median lay below the one-lane leg's
    minimum) left the chains on sha512_pair_max_groups(): the header spells no
    threshold of their own, and the unit routes by that function."""
    with open(os.path.join(CSRC, "mirsha_sha512_chains.h")) as f:
        assert not re.search(r"constexpr uint32_t k\w*MaxGroups", f.read())
    with open(os.path.join(ROOT, NEW_UNIT)) as f:
        unit = f.read()
    assert re.search(r"<= sha512_pair_max_groups\(\)", unit) and "getenv" not in unit


def _git(*args):
    return subprocess.run(["git", *args], cwd=ROOT, capture_output=True, text=True)


def test_kernel_sources_untouched_by_the_chains_pair_route():
    """The change that added mirsha_sha512_chains_pair.hip must not differ from
    its parent in any of the seven files (while that change is not committed
    yet, the parent is HEAD)."""
    assert os.path.exists(os.path.join(ROOT, NEW_UNIT))
    if _git("rev-parse", "--is-inside-work-tree").stdout.strip() != "true":
        pytest.skip("not a git checkout")
    added = _git("log", "--diff-filter=A", "--format=%H", "--", NEW_UNIT).stdout.split()
    if added:
        parent = _git("rev-parse", "--verify", "--quiet", added[-1] + "~")
        if parent.returncode != 0:
            pytest.skip("the parent commit is not in this checkout (shallow clone)")
        r = _git("diff", "--quiet", parent.stdout.strip(), added[-1], "--", *UNTOUCHED)
    else:
        r = _git("diff", "--quiet", "HEAD", "--", *UNTOUCHED)
    assert r.returncode == 0, "a kernel source differs from the parent commit's"
