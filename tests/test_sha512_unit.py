"""CPU unit test of the host-compilable core of mirbft_amd/csrc/sha512_device.h
(tests/c/sha512_unit.cpp, built with g++ -- no HIP): the SHA-512/256
compression, the padding of a message's blocks and the blocks of a digest list,
driven the way the two kernels drive them.  The expected digests come from
hashlib.  Built twice, as tests/test_stream_seg_unit.py builds its program:
optimised, and with AddressSanitizer + UndefinedBehaviorSanitizer (host code
only, a stand-alone program run directly)."""
import hashlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL = -1


def h(b: bytes) -> str:
    return hashlib.new("sha512_256", b).hexdigest()


def msg(length: int) -> bytes:  # sha512_unit.cpp: msg_byte
    return bytes((i * 131 + length * 7 + 13) & 0xFF for i in range(length))


def row(r: int) -> bytes:  # sha512_unit.cpp: row_byte
    return bytes((r * 37 + j * 11 + 5) & 0xFF for j in range(32))


def list_cases():
    """List sizes 0..9, plain and with nulls at head, middle and tail (and all
    null); a repeated and a descending index ride along."""
    cases = []
    for n in range(10):
        ids = [(7 * k + 3) % 50 for k in range(n)]
        cases.append(ids)
        cases.append([NULL] + ids)
        cases.append(ids + [NULL])
        cases.append(ids[: n // 2] + [NULL, NULL] + ids[n // 2:])
        cases.append([NULL] * n)
    cases.append([9, 9, 9, 9, 9])
    cases.append([8, 7, 6, 5, 4, 3, 2, 1, 0])
    return cases


def cases_text() -> str:
    lines = []
    for length in list(range(301)) + [1000, 65535, 65536]:  # crosses 111/112, 127/128, 239/240
        lines.append(f"M {length} {h(msg(length))}")
    fips896 = (b"abcdefghbcdefghicdefghijdefghijkefghijklfghijklmghijklmnhijklmno"
               b"ijklmnopjklmnopqklmnopqrlmnopqrsmnopqrstnopqrstu")
    vectors = {b"": "c672b8d1ef56ed28ab87c3622c5114069bdd3ad7b8f9737498d0c01ecef0967a",
               b"abc": "53048e2681941ef99b2e29b76b4c7dabe4c2d0c634fc6d46e0e2f13107e7af23",
               fips896: "3928e184fb8690f840da3988121d31be65cb9d3ef83ee6146feac861e19b563a"}
    for m, want in vectors.items():  # FIPS 180-4 / NIST example values, literal
        assert h(m) == want
        lines.append(f"S {m.hex() or '-'} {want}")
    for ids in list_cases():
        want = h(b"".join(row(i) for i in ids if i != NULL))
        lines.append(" ".join(["L", str(len(ids)), *map(str, ids), want]))
    return "\n".join(lines) + "\n"


def _build_and_run(tmp_path, name, flags, env=None):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mirbft_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "sha512_unit.cpp"), "-o", exe], check=True)
    cases = tmp_path / (name + ".cases")
    text = cases_text()
    cases.write_text(text)
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.strip() == f"sha512 unit ok: {text.count(chr(10))} cases"


def test_sha512_core(tmp_path):
    _build_and_run(tmp_path, "sha512_unit", ["-O2"])


def test_sha512_core_sanitized(tmp_path):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "p")],
                           input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("g++ without ASan/UBSan runtime")
    _build_and_run(tmp_path, "sha512_unit_asan",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer"],
                   # a preloaded library (some sandboxes add one) must not stop ASan at startup
                   env=dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0"))
