"""CPU unit test of mirbft_amd/csrc/sha512_pair.h (tests/c/sha512_pair_unit.cpp,
built with g++ -- no HIP): the SHA-512 compression split into producer and
consumer, driven through a two-slot ring in the order of the pair kernels
(producer one group of 16 rounds ahead, slots alternating, a dead lane's block
not added), and produce_kw + consume_kw == sha512::compress on random states
and words.  The cases are those of tests/test_sha512_unit.py (every message
length 0..300, 1000, 65535, 65536, the FIPS vectors, its list cases with
nulls); the expected digests come from hashlib.  Built and run the way that test
builds its program: optimised, and with AddressSanitizer +
UndefinedBehaviorSanitizer (host code only, a stand-alone program run
directly)."""
import os
import subprocess

import pytest

from test_sha512_unit import cases_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, name, flags, env=None):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mirbft_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "sha512_pair_unit.cpp"), "-o", exe], check=True)
    cases = tmp_path / (name + ".cases")
    text = cases_text()
    cases.write_text(text)
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.strip() == f"sha512 pair unit ok: {text.count(chr(10))} cases"


def test_sha512_pair_split(tmp_path):
    _build_and_run(tmp_path, "sha512_pair_unit", ["-O2"])


def test_sha512_pair_split_sanitized(tmp_path):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "p")],
                           input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("g++ without ASan/UBSan runtime")
    _build_and_run(tmp_path, "sha512_pair_unit_asan",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer"],
                   # a preloaded library (some sandboxes add one) must not stop ASan at startup
                   env=dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0"))
