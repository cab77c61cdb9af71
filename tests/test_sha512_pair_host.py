"""Host-side surface of the SHA-512/256 pair route (no GPU): the two entries
that show the route, the threshold with and without the A/B knobs, and that the
change which brought the route left the one-lane SHA-512/256 units and the
SHA-256 kernel sources (the inputs of bench.py's traffic_key) byte for byte
alone."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

import mirbft_amd
from mirbft_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNTOUCHED = ["mirbft_amd/csrc/mirsha_kernels.hip", "mirbft_amd/csrc/mirsha_kernels.h",
             "mirbft_amd/csrc/sha256_device.h", "mirbft_amd/csrc/sha256_rounds_asm.h",
             "mirbft_amd/csrc/mirsha_sha512.hip", "mirbft_amd/csrc/mirsha_sha512_plan.hip"]
NEW_UNIT = "mirbft_amd/csrc/mirsha_sha512_pair.hip"
KNOBS = ("MIRSHA_AB", "MIRSHA_SHA512_PAIR", "MIRSHA_SHA512_PAIR_MAX_GROUPS")


def test_names_are_bound_with_the_headers_arity():
    with open(os.path.join(ROOT, "include", "mirsha.h")) as f:
        header = f.read()
    for name, arity in (("mirsha_sha512_pair_max_groups", 0), ("mirsha_ctx_sha512_pair_launches", 2)):
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert m, name
        params = [] if m.group(1).strip() == "void" else m.group(1).split(",")
        assert len(params) == arity
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == arity
        assert hasattr(_lib.load(), name)
    assert "sha512_pair_max_groups" in mirbft_amd.__all__
    assert isinstance(mirbft_amd.Engine.sha512_pair_launches, property)


def test_pair_launches_null_answers():
    lib = _lib.load()
    n = ctypes.c_uint64(7)
    assert lib.mirsha_ctx_sha512_pair_launches(None, ctypes.byref(n)) == _lib.MIRSHA_EINVAL
    assert lib.mirsha_ctx_sha512_pair_launches(None, None) == _lib.MIRSHA_EINVAL
    assert n.value == 7


def _threshold_in_a_child(**knobs) -> int:
    """The threshold is read once per process, so each setting gets its own."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs)
    r = subprocess.run([sys.executable, "-c",
                        "import sys; sys.path.insert(0, sys.argv[1]); import mirbft_amd; "
                        "print(mirbft_amd.sha512_pair_max_groups())", ROOT],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return int(r.stdout.strip())


# The derivation gives 512 (half of the chip's 1,024 SIMDs); the measurement's
# decision rule (the largest measured group count at which the
# pair's median lay below the parent's min-max) lowered it to 256.
DEFAULT = 256


def test_threshold_default_and_the_knobs_only_with_ab():
    with open(os.path.join(ROOT, "mirbft_amd", "csrc", "mirsha_sha512_pair.h")) as f:
        m = re.search(r"constexpr uint32_t kSha512PairMaxGroups = (\d+);", f.read())
    assert m and int(m.group(1)) == DEFAULT
    if not any(k in os.environ for k in KNOBS):
        assert _lib.load().mirsha_sha512_pair_max_groups() == DEFAULT
        assert mirbft_amd.sha512_pair_max_groups() == DEFAULT
    assert _threshold_in_a_child() == DEFAULT
    assert _threshold_in_a_child(MIRSHA_AB="1", MIRSHA_SHA512_PAIR_MAX_GROUPS="3") == 3
    assert _threshold_in_a_child(MIRSHA_AB="1", MIRSHA_SHA512_PAIR="0") == 0
    assert _threshold_in_a_child(MIRSHA_AB="1", MIRSHA_SHA512_PAIR="0", MIRSHA_SHA512_PAIR_MAX_GROUPS="3") == 0
    # without MIRSHA_AB=1 the knobs are not read
    assert _threshold_in_a_child(MIRSHA_SHA512_PAIR_MAX_GROUPS="3") == DEFAULT
    assert _threshold_in_a_child(MIRSHA_SHA512_PAIR="0") == DEFAULT
    assert _threshold_in_a_child(MIRSHA_AB="0", MIRSHA_SHA512_PAIR="0") == DEFAULT


def _git(*args):
    return subprocess.run(["git", *args], cwd=ROOT, capture_output=True, text=True)


def test_kernel_sources_untouched_by_the_pair_route():
    """The change that added mirsha_sha512_pair.hip must not differ from its
    parent in any of the six files (while that change is not committed yet, the
    parent is HEAD)."""
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
