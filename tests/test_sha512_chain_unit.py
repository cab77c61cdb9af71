"""CPU unit test of the host-compilable step of a SHA-512/256 commit programme
(mirbft_amd/csrc/sha512_chain.h through tests/c/sha512_chain_unit.cpp, built
with g++ -- no HIP): planning a step from entries and count, and building the
block from pending rows, new rows, marker and length, driven the way the
kernels of mirsha_sha512_chains.hip drive them.  The program prints every
checkpoint value and the sum of the state left behind; the expected values come
from hashlib.  Built twice, as tests/test_sha512_unit.py builds its program:
optimised, and with AddressSanitizer + UndefinedBehaviorSanitizer (host code
only, a stand-alone program run directly)."""
import hashlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CP = -1
EMPTY = "c672b8d1ef56ed28ab87c3622c5114069bdd3ad7b8f9737498d0c01ecef0967a"


def row(r: int) -> bytes:  # sha512_chain_unit.cpp: row_byte
    return bytes((r * 37 + j * 11 + 5) & 0xFF for j in range(32))


def expected(p, ops):
    """hashlib restatement: the checkpoint values, then the final sum twice."""
    h = hashlib.new("sha512_256")
    for i in range(p):
        h.update(row(1000 + i))
    out = []
    for op in ops:
        if op == CP:
            out.append(h.hexdigest())
            h = hashlib.new("sha512_256")
        else:
            h.update(row(op))
    return out + [h.hexdigest()] * 2


def programmes():
    """(p, ops): every class (p, a, m, b), the programmes without a checkpoint,
    back-to-back checkpoints on a fresh state, one long programme."""
    progs = []
    ids = iter(range(10 ** 9))

    def writes(k):
        return [next(ids) % 997 for _ in range(k)]

    for p in range(4):
        for a in range(6):
            for m in [None] + list(range(6)):
                for b in range(6):
                    ops = writes(a) + [CP]
                    if m is not None:
                        ops += writes(m) + [CP]
                    progs.append((p, ops + writes(b)))
        for k in range(10):
            progs.append((p, writes(k)))
    progs.append((0, [CP, CP]))
    progs.append((0, [CP, CP, CP] + writes(1)))
    progs.append((0, writes(1000)))
    progs.append((3, writes(500) + [CP] + writes(499) + [CP]))
    return progs


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mirbft_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "sha512_chain_unit.cpp"), "-o", exe], check=True)
    return exe


def _run(tmp_path, name, flags, env=None):
    exe = _build(tmp_path, name, flags)
    progs = programmes()
    lines = [" ".join([mode, str(p), str(len(ops)), *map(str, ops)]) for mode in "UC" for p, ops in progs]
    cases = tmp_path / (name + ".cases")
    cases.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    got = [line.split() for line in r.stdout.splitlines()]
    assert len(got) == 2 * len(progs)
    for k, words in enumerate(got):
        mode, (p, ops) = "UC"[k // len(progs)], progs[k % len(progs)]
        assert words == expected(p, ops), (mode, p, ops[:40])
    # SHA-512/256 of the empty message, literally: two checkpoints back to back on a fresh state
    k = progs.index((0, [CP, CP]))
    assert got[k] == [EMPTY] * 4 and got[len(progs) + k] == [EMPTY] * 4


def test_sha512_chain_step(tmp_path):
    _run(tmp_path, "sha512_chain_unit", ["-O2"])


def test_sha512_chain_step_sanitized(tmp_path):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "p")],
                           input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("g++ without ASan/UBSan runtime")
    _run(tmp_path, "sha512_chain_unit_asan",
         ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
         # a preloaded library (some sandboxes add one) must not stop ASan at startup
         env=dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0"))
