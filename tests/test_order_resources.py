"""Resources of the order kernels (CPU: hipcc's resource-usage remarks for
gfx950, device code only, as tests/test_chains_resources.py does for the
commits' segment kernel).  The count and scatter kernels are one wave per
workgroup walking its chunk; a spill to scratch would put memory round trips
into the scatter's match loop."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mirbft_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("order_count_kernel", "order_scatter_kernel", "order_iota_kernel")


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("res") / "order.o"
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "--cuda-device-only", "-c", "mirsha_order.hip", "-o", str(out),
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
def test_order_kernels_have_no_scratch_and_no_spills(resources, kernel):
    hits = {k: v for k, v in resources.items() if kernel in k}
    assert len(hits) == 1, sorted(resources)
    (res,) = hits.values()
    assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, res
    # the histogram is dynamic LDS (4 bytes per bin), nothing static
    assert res["LDS Size"] == 0, res


def test_the_unit_holds_only_the_order_kernels(resources):
    """The hashing kernels stay in their own code object (mirsha_kernels.hip)."""
    assert len(resources) == len(KERNELS), sorted(resources)
    assert all(any(k in name for k in KERNELS) for name in resources), sorted(resources)
