"""Register budget of the checkpoint-chain kernels (CPU: hipcc's resource-usage
remarks for gfx950, device code only, as tests/test_kernel_resources.py does
for mirsha_kernels.hip).  chains_commit_seg_kernel is one latency-bound wave of
dependent compressions: a spill to scratch would put memory round trips into
every round."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mirbft_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

CHAIN_KERNELS = ("chains_absorb_kernel", "chains_sum_kernel", "chains_reset_kernel", "chains_commit_kernel",
                 "chains_commit_seg_kernel")


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("res") / "cr.o"
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "--cuda-device-only", "-c", "mirsha_chains.hip", "-o", str(out),
                        "-Rpass-analysis=kernel-resource-usage"],
                       cwd=CSRC, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    assert kernels, r.stderr[-2000:]
    return kernels


def test_segment_kernel_has_no_scratch_and_no_spills(resources):
    hits = {k: v for k, v in resources.items() if "chains_commit_seg_kernel" in k}
    assert len(hits) == 1, sorted(resources)
    (res,) = hits.values()
    assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, res
    # the synchronous kernel's budget (86 VGPRs); the wave keeps at least 4 per SIMD
    assert res["VGPRs"] <= 128 and res["Occupancy"] >= 4, res


def test_no_scratch_or_spills(resources):
    """Every kernel of the unit, as test_kernel_resources.py asserts of mirsha_kernels.hip's."""
    bad = {k: v for k, v in resources.items()
           if v.get("ScratchSize", 0) or v.get("VGPRs Spill", 0)}
    assert not bad, f"kernels spilling to scratch: {bad}"


def test_the_unit_holds_the_chain_kernels_and_no_other(resources):
    """The hashing kernels stay in their own code object (mirsha_kernels.hip;
    tests/test_kernel_resources.py asserts that it holds no chain kernel)."""
    names = sorted(re.match(r"_ZN6mirsha\d+([a-z_]+_kernel)E", k).group(1) if k.startswith("_ZN6mirsha") else k
                   for k in resources)
    assert names == sorted(CHAIN_KERNELS), names
