"""Register budget of the hinted request kernel (CPU: hipcc's resource-usage
remarks for gfx950, device code only, ~5 s).

sha256_msgs_kernel<true, false, true> holds two tile functions, hash_tile_uniform
and hash_tile, and hash_tile alone fills the 64-VGPR / 80-SGPR budget of 8 waves
per SIMD (tests/test_kernel_resources.py pins the occupancy and the scratch of
every kernel of the unit, this one included).  What that file does not see:
SGPR spills go to VGPR lanes, not to scratch, and cost v_writelane /
v_readlane pairs on the path the hint exists to shorten."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mirbft_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
HINTED = "sha256_msgs_kernelILb1ELb0ELb1E"
UNHINTED = "sha256_msgs_kernelILb1ELb0ELb0E"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("hintres") / "k.o"
    r = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "--cuda-device-only", "-c", "mirsha_kernels.hip", "-o", str(out),
                        "-Rpass-analysis=kernel-resource-usage"],
                       cwd=CSRC, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    found, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = found.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return found


@pytest.mark.parametrize("name", [HINTED, UNHINTED])
def test_request_kernel_budget(kernels, name):
    hits = [v for k, v in kernels.items() if name in k]
    assert len(hits) == 1, sorted(kernels)
    v = hits[0]
    assert v["VGPRs"] <= 64 and v["Occupancy"] >= 8, v
    assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, v
