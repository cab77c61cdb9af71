"""CPU unit test of the host-compilable step of a stream programme under
SHA-512/256 (mirbft_amd/csrc/sha512_stream.h through
tests/c/sha512_stream_unit.cpp, built with g++ -- no HIP): the plan of a step,
the merge of a 128-byte window under a byte mask, the padding of a Sum over one
or two blocks, driven over a byte arena by a host loader that gives zero outside
[0, span), the way the kernels of mirsha_sha512_streams.hip drive it.  The
program prints every sum's value; the expected values come from hashlib.  Built
twice, as tests/test_sha512_chain_unit.py builds its program: optimised, and
with AddressSanitizer + UndefinedBehaviorSanitizer (host code only, a
stand-alone program run directly)."""
import hashlib
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, SUM, SUM_RESET, RESET = 0, 1, 2, 3
EMPTY = "c672b8d1ef56ed28ab87c3622c5114069bdd3ad7b8f9737498d0c01ecef0967a"
ARENA = 6000
BYTES = bytes((j * 131 + 7 + (j >> 8) * 17) & 0xFF for j in range(ARENA))  # sha512_stream_unit.cpp: arena_byte
SUM_TOTALS = (0, 1, 111, 112, 113, 127, 128, 239, 240, 256)


def grid_lengths(b):
    return sorted({n for n in (0, 1, 127 - b, 128 - b, 129 - b, 128, 129, 255, 256, 257) if n >= 0})


def expected(arena_len, ops):
    h = hashlib.new("sha512_256")
    out = []
    for kind, off, ln in ops:
        if kind == W:
            assert ln > 0 and off + ln <= arena_len
            h.update(BYTES[off:off + ln])
        if kind in (SUM, SUM_RESET):
            out.append(h.hexdigest())
        if kind in (SUM_RESET, RESET):
            h = hashlib.new("sha512_256")
    return out


def cases():
    """(shift, arena_len, ops); ops = (kind, off, len).  A zero-length write is
    dropped by the plan and never reaches a step, so it is dropped here too."""
    out = []

    def writes(*ranges):
        return [(W, off, ln) for off, ln in ranges if ln]

    for shift in range(4):
        for b in range(128):
            for n in grid_lengths(b):
                # the stream arrives at fill b, then takes n bytes from another place
                out.append((shift, 700, writes((3, b), (200 + b % 5, n)) + [(SUM, 0, 0)]))
        for b in (1, 5, 64, 126, 127):
            for n in (1, 3, 128 - b, 129, 300):
                # a write at arena offset 0 arriving at a fill: the window begins before the arena
                out.append((shift, 400, writes((17, b), (0, n)) + [(SUM, 0, 0)]))
                # a write that ends at the arena's last byte
                out.append((shift, 400, writes((17, b), (400 - n, n)) + [(SUM, 0, 0)]))
        out.append((shift, 1, writes((0, 1)) + [(SUM, 0, 0)]))
        for t in SUM_TOTALS:
            # summed twice (the state is untouched), written on, summed again
            out.append((shift, 600, writes((5, t)) + [(SUM, 0, 0), (SUM, 0, 0)] + writes((300, 77)) + [(SUM, 0, 0)]))
            out.append((shift, 600, writes((5, t)) + [(SUM_RESET, 0, 0)] + writes((9, 130)) + [(SUM, 0, 0)]))
            out.append((shift, 600, writes((5, t)) + [(RESET, 0, 0)] + writes((9, t)) + [(SUM_RESET, 0, 0), (SUM, 0, 0)]))
    rng = random.Random(512)
    ops, at = [], 0
    while at < 5000:  # one 5,000-byte message cut into random writes, summed on the way
        n = min(rng.choice((1, 2, 7, 63, 64, 65, 127, 128, 129, 300, 700)), 5000 - at)
        ops.append((W, 11 + at, n))
        at += n
        if rng.random() < 0.2:
            ops.append((SUM, 0, 0))
    out.append((1, ARENA, ops + [(SUM, 0, 0)]))
    out.append((0, 0, [(SUM, 0, 0), (SUM_RESET, 0, 0), (SUM, 0, 0)]))  # the empty message
    return out


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mirbft_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "sha512_stream_unit.cpp"), "-o", exe], check=True)
    return exe


def _run(tmp_path, name, flags, env=None):
    exe = _build(tmp_path, name, flags)
    cs = cases()
    lines = [" ".join([mode, str(shift), str(alen), str(len(ops)), *(str(v) for op in ops for v in op)])
             for mode in "UC" for shift, alen, ops in cs]
    path = tmp_path / (name + ".cases")
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    got = [line.split() for line in r.stdout.splitlines()]
    assert len(got) == 2 * len(cs)
    for k, words in enumerate(got):
        mode, (shift, alen, ops) = "UC"[k // len(cs)], cs[k % len(cs)]
        assert words == expected(alen, ops), (mode, shift, alen, ops[:12])
    assert got[len(cs) - 1] == [EMPTY] * 3 and got[-1] == [EMPTY] * 3  # literally


def test_sha512_stream_step(tmp_path):
    _run(tmp_path, "sha512_stream_unit", ["-O2"])


def test_sha512_stream_step_sanitized(tmp_path):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "p")],
                           input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("g++ without ASan/UBSan runtime")
    _run(tmp_path, "sha512_stream_unit_asan",
         ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
         # a preloaded library (some sandboxes add one) must not stop ASan at startup
         env=dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0"))
