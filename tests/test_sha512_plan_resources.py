"""Resources of the SHA-512/256 plan kernels (CPU: hipcc's resource-usage
remarks for gfx950, device code only, as tests/test_sha512_resources.py does
for the two kernels of mirsha_sha512.hip).  The plan-form list walk keeps two
blocks of rows, the schedule window and the state in registers with static
indices, and the overlapped kernel holds that walk twice beside the message
lane: a runtime-indexed register array would go to scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mirbft_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# as the remarks spell them: the mangled names of the two instances and the kernel
KERNELS = ("sha512_plan_lists_kernelILb0EE", "sha512_plan_lists_kernelILb1EE", "sha512_overlap_kernel")


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("res") / "sha512_plan.o"
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "--cuda-device-only", "-c", "mirsha_sha512_plan.hip", "-o", str(out),
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
def test_plan_kernel_has_no_scratch_no_spills_no_lds(resources, kernel):
    hits = {k: v for k, v in resources.items() if kernel in k}
    assert len(hits) == 1, sorted(resources)
    (res,) = hits.values()
    print(kernel, res)  # the VGPR counts are recorded in DESIGN.md 1.6, not asserted
    assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, res
    assert res["LDS Size"] == 0, res


def test_the_unit_holds_exactly_its_three_kernels(resources):
    """The request and list kernels of the other calls stay in mirsha_sha512.hip,
    the SHA-256 kernels in their own code objects."""
    assert len(resources) == len(KERNELS), sorted(resources)
    assert all(any(k in name for k in KERNELS) for name in resources), sorted(resources)
