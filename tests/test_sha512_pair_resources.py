"""Resources of the SHA-512/256 producer/consumer pair kernels (CPU: hipcc's
resource-usage remarks for gfx950, device code only, as
tests/test_sha512_resources.py does for the one-lane kernels).  A kernel holds
the producer's block loads and schedule window and the consumer's state and
working variables, every index static: a runtime-indexed register array would
go to scratch.  The ring is static LDS, so it has to fit 64 KiB without a
dynamic-LDS attribute call."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mirbft_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# as the remarks spell them: the kernels and the mangled names of the two instances
KERNELS = ("sha512_msgs_pair_kernel", "sha512_lists_pair_kernel", "sha512_plan_lists_pair_kernelILb0EE",
           "sha512_plan_lists_pair_kernelILb1EE")


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("res") / "sha512_pair.o"
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "--cuda-device-only", "-c", "mirsha_sha512_pair.hip", "-o", str(out),
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


@pytest.mark.parametrize("kernel", KERNELS)
def test_pair_kernel_has_no_scratch_no_spills_and_a_static_ring(resources, kernel):
    hits = {k: v for k, v in resources.items() if kernel in k}
    assert len(hits) == 1, sorted(resources)
    (res,) = hits.values()
    print(kernel, res)  # the VGPR and SGPR counts are recorded in DESIGN.md 1.6, not asserted
    assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, res
    assert 0 < res["LDS Size"] <= 65536, res


def test_the_unit_holds_exactly_its_kernels(resources):
    """The one-lane kernels stay in mirsha_sha512.hip and mirsha_sha512_plan.hip,
    the SHA-256 kernels in their own code objects."""
    assert len(resources) == len(KERNELS), sorted(resources)
    assert all(any(k in name for k in KERNELS) for name in resources), sorted(resources)
