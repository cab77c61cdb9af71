"""Resources of the gathering select kernel (CPU: hipcc's resource-usage remarks
for gfx950, device code only, as tests/test_chains_resources.py does for
mirsha_chains.hip).  expect_select_gather_kernel is one lane per request
with five loads and two stores: scratch, a spill or LDS would mean the
compiler did not keep the two digest words in registers across the ballot."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mirbft_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("res") / "xp.o"
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "--cuda-device-only", "-c", "mirsha_expect.hip", "-o", str(out),
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


def test_gather_kernel_has_no_scratch_no_spills_and_no_lds(resources):
    hits = {k: v for k, v in resources.items() if "expect_select_gather_kernel" in k}
    assert len(hits) == 1, sorted(resources)
    (res,) = hits.values()
    assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, res
    assert res["LDS Size"] == 0, res


def test_the_unit_holds_the_two_select_kernels_only(resources):
    """The hashing kernels stay in their own code object (mirsha_kernels.hip)."""
    assert len(resources) == 2 and all("expect_select" in k for k in resources), sorted(resources)
