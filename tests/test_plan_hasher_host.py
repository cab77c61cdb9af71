"""Host-side surface of the plans' hasher (no GPU): the NULL answer of
mirsha_pipeline_hasher, the binding table against the header, and that the
change which brought the SHA-512/256 plans left the SHA-256 kernel sources (the
inputs of bench.py's kernel_source_key) byte for byte alone."""
import os
import re
import subprocess

import pytest

from mirbft_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHA256_KERNEL_SOURCES = ["mirbft_amd/csrc/mirsha_kernels.hip", "mirbft_amd/csrc/mirsha_kernels.h",
                         "mirbft_amd/csrc/sha256_device.h", "mirbft_amd/csrc/sha256_rounds_asm.h"]
NEW_UNIT = "mirbft_amd/csrc/mirsha_sha512_plan.hip"


def test_pipeline_hasher_of_null_is_einval():
    assert _lib.load().mirsha_pipeline_hasher(None) == _lib.MIRSHA_EINVAL


def test_names_are_bound_with_the_headers_arity():
    with open(os.path.join(ROOT, "include", "mirsha.h")) as f:
        header = f.read()
    for name, arity in (("mirsha_pipeline_create_hasher", 9), ("mirsha_pipeline_hasher", 1)):
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == arity
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == arity
        assert hasattr(_lib.load(), name)


def _git(*args):
    return subprocess.run(["git", *args], cwd=ROOT, capture_output=True, text=True)


def test_sha256_kernel_sources_untouched_by_the_plans_change():
    """The change that added mirsha_sha512_plan.hip must not differ from its
    parent in any of the four files (while that change is not committed yet,
    the parent is HEAD)."""
    assert os.path.exists(os.path.join(ROOT, NEW_UNIT))
    if _git("rev-parse", "--is-inside-work-tree").stdout.strip() != "true":
        pytest.skip("not a git checkout")
    added = _git("log", "--diff-filter=A", "--format=%H", "--", NEW_UNIT).stdout.split()
    if added:
        parent = _git("rev-parse", "--verify", "--quiet", added[-1] + "~")
        if parent.returncode != 0:
            pytest.skip("the parent commit is not in this checkout (shallow clone)")
        r = _git("diff", "--quiet", parent.stdout.strip(), added[-1], "--", *SHA256_KERNEL_SOURCES)
    else:
        r = _git("diff", "--quiet", "HEAD", "--", *SHA256_KERNEL_SOURCES)
    assert r.returncode == 0, "a SHA-256 kernel source differs from the parent commit's"
