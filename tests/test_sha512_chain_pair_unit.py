"""CPU unit test of mirbft_amd/csrc/sha512_chain_pair.h
(tests/c/sha512_chain_pair_unit.cpp, built with g++ -- no HIP): the step of a
SHA-512/256 commit programme split into the producer's walk and the consumer's
rounds, for 64 lanes in lock-step through a host array shaped like the ring of
mirsha_sha512_chains_pair.hip.  The program stamps every ring slot and control
word with the phase of its writing and reading, counts both roles' barriers, and
compares every checkpoint row and the final state with the one-lane walk
(sha512::chain_plan / chain_block / compress): every count of pending rows
against every kind of step, consecutive checkpoints, empty programmes, and 200
random groups of 64 programmes of 0-40 entries.  Built and run the way
tests/test_sha512_pair_unit.py builds its program: optimised, and with
AddressSanitizer + UndefinedBehaviorSanitizer (host code only, a stand-alone
program run directly)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, name, flags, env=None):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mirbft_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "sha512_chain_pair_unit.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    m = re.fullmatch(r"sha512 chain pair unit ok: (\d+) groups", r.stdout.strip())
    # one group of all step classes, 34 of a class alone, consecutive checkpoints, two empty, 200 random
    assert m and int(m.group(1)) == 1 + 34 + 1 + 2 + 200, r.stdout


def test_sha512_chain_pair_step(tmp_path):
    _build_and_run(tmp_path, "sha512_chain_pair_unit", ["-O2"])


def test_sha512_chain_pair_step_sanitized(tmp_path):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "p")],
                           input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("g++ without ASan/UBSan runtime")
    _build_and_run(tmp_path, "sha512_chain_pair_unit_asan",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer"],
                   # a preloaded library (some sandboxes add one) must not stop ASan at startup
                   env=dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0"))
