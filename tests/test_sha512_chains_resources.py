"""Resources of the SHA-512/256 checkpoint-chain kernels (CPU: hipcc's
resource-usage remarks for gfx950, device code only, as
tests/test_sha512_resources.py does for the request and list kernels).  The
commit kernels keep the state, 12 pending words, the block, the schedule window
and a prefetched step in registers with static indices: a runtime-indexed
register array would go to scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mirbft_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("sha512_chains_commit_kernel", "sha512_chains_sum_kernel", "sha512_chains_reset_kernel",
           "sha512_chains_commit_seg_kernel")


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("res") / "sha512_chains.o"
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "--cuda-device-only", "-c", "mirsha_sha512_chains.hip", "-o", str(out),
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
def test_chains_kernel_has_no_scratch_no_spills_no_lds(resources, kernel):
    hits = {k: v for k, v in resources.items() if re.search(r"\d" + kernel + "E", k)}
    assert len(hits) == 1, sorted(resources)
    (res,) = hits.values()
    print(kernel, res)  # the VGPR counts are recorded in DESIGN.md 1.6, not asserted
    assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, res
    assert res["LDS Size"] == 0, res


def test_the_unit_holds_only_its_four_kernels(resources):
    """The other kernels stay in their own code objects."""
    assert len(resources) == len(KERNELS), sorted(resources)
    assert all(any(re.search(r"\d" + k + "E", name) for k in KERNELS) for name in resources), sorted(resources)
