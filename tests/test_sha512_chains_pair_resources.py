"""Resources of the pair forms of the SHA-512/256 checkpoint-chain commit
kernels (CPU: hipcc's resource-usage remarks for gfx950, device code only, as
tests/test_sha512_pair_resources.py does for the request and list pair
kernels).  A kernel holds the producer's walk (the pending words, a prefetched
step of four entries and eight 128-bit rows, the schedule window) and the
consumer's state and working variables, every index static: a runtime-indexed
register array would go to scratch.  The ring is static LDS, so it has to fit
64 KiB without a dynamic-LDS attribute call."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mirbft_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("sha512_chains_commit_pair_kernel", "sha512_chains_commit_seg_pair_kernel")


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("res") / "sha512_chains_pair.o"
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "--cuda-device-only", "-c", "mirsha_sha512_chains_pair.hip", "-o", str(out),
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
def test_chains_pair_kernel_has_no_scratch_no_spills_and_a_static_ring(resources, kernel):
    hits = {k: v for k, v in resources.items() if re.search(r"\d" + kernel + "E", k)}
    assert len(hits) == 1, sorted(resources)
    (res,) = hits.values()
    print(kernel, res)  # the VGPR and SGPR counts are recorded in DESIGN.md 1.6, not asserted
    assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, res
    assert 0 < res["LDS Size"] <= 65536, res


def test_the_unit_holds_exactly_its_kernels(resources):
    """The one-lane kernels stay in mirsha_sha512_chains.hip, the request and
    list pair kernels in mirsha_sha512_pair.hip."""
    assert len(resources) == len(KERNELS), sorted(resources)
    assert all(any(re.search(r"\d" + k + "E", name) for k in KERNELS) for name in resources), sorted(resources)
