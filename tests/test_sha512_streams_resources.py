"""Resources of the SHA-512/256 stream kernels (CPU: hipcc's resource-usage
remarks for gfx950, device code only, as tests/test_streams_ring_resources.py
does for streams_seg_kernel).  Both kernels walk a programme by the step of
sha512_stream.h: the block in 32 named registers, any byte range merged under
masks; a runtime-indexed register array would go to scratch, and a spill would
put memory round trips into every step."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mirbft_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("sha512_streams_kernel", "sha512_streams_seg_kernel")


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("res") / "sha512_streams.o"
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "--cuda-device-only", "-c", "mirsha_sha512_streams.hip", "-o", str(out),
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
def test_stream_kernel_has_no_scratch_and_no_spills(resources, kernel):
    hits = {k: v for k, v in resources.items() if re.search(r"\d" + kernel + "E", k)}
    assert len(hits) == 1, sorted(resources)
    (res,) = hits.values()
    print(res)  # the VGPR / AGPR counts are recorded in DESIGN.md 1.5.2, not asserted
    assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, res
    assert res["LDS Size"] == 0, res


def test_the_unit_holds_only_the_two_stream_kernels(resources):
    """The hashing kernels stay in their own code objects, and so do the SHA-256
    stream kernels and the SHA-512/256 chain kernels."""
    assert len(resources) == len(KERNELS), sorted(resources)
    assert all(any(k in name for k in KERNELS) for name in resources), sorted(resources)
