"""The host-side hint set of a uniform request launch (mirsha_hints.h).

make_uniform_hint(L, stride) derives, from the length alone, what the request
kernel otherwise works out per wave: the block count, whether the final block
takes the tail form, the tail form's keep / mark words and the TailWords
scalars that tail_words() (sha256_device.h) computes on the device.  Here every
field is checked for L in 0..600 against the padded message itself: the final
block is built byte by byte as FIPS 180-4 section 5.1.1 says (data, 0x80,
zeros, 64-bit bit length), and the expected scalars are read off its words.
Plain C++ and Python: no GPU.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LEN = 600
M32 = 0xFFFFFFFF
K4, K14, K15 = 0x3956C25B, 0x9BDC06A7, 0xC19BF174  # FIPS 180-4 section 4.2.2


def _rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & M32


def _ssig0(x):
    return _rotr(x, 7) ^ _rotr(x, 18) ^ (x >> 3)


def _ssig1(x):
    return _rotr(x, 17) ^ _rotr(x, 19) ^ (x >> 10)


def _final_block(L):
    """(block count, words of the final block with every data byte 0xFF, the same
    with every data byte 0x00) of an L-byte message."""
    def words(fill):
        m = bytes([fill]) * L + b"\x80"
        m += b"\x00" * (-(len(m) + 8) % 64) + (8 * L).to_bytes(8, "big")
        assert len(m) % 64 == 0
        last = m[-64:]
        return len(m) // 64, [int.from_bytes(last[4 * k:4 * k + 4], "big") for k in range(16)]

    nb, ones = words(0xFF)
    _, zeros = words(0x00)
    return nb, ones, zeros


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hint") / "uniform_hint_unit")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "mirbft_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "uniform_hint_unit.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(MAX_LEN), "L", "4096", "0", "6", str(1 << 32), str((1 << 32) - 4)],
                       capture_output=True, text=True, check=True, timeout=60)
    out = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
    assert len(out) == 6 * (MAX_LEN + 1)
    return out


def test_hint_scalars_match_fips_padding(rows):
    seen_tail = seen_plain = seen_len_only = 0
    for row in rows:
        L, stride, valid = row[0], row[1], row[2]
        if stride % 4 or stride > M32:
            assert valid == 0, (L, stride)
            continue
        (_, _, _, ln, st, nb, loop_nb, tail, tail_bytes, tail_pad, reach) = row[:11]
        keep, mark, tw = row[11:15], row[15:19], row[19:30]
        assert (valid, ln, st) == (1, L, stride)
        want_nb, ones, zeros = _final_block(L)
        assert nb == want_nb == (L + 72) >> 6, L
        u = L - 64 * (nb - 1)  # message bytes in the final block; < 0: the 0x80 went into the block before
        assert tail == (1 if u <= 16 else 0), L
        assert loop_nb == (nb - 1 if tail else nb), L
        assert tail_bytes == (1 if tail and u > 0 else 0), L
        assert tail_pad == (1 if tail and u < 16 else 0), L
        # every byte the loads touch, and no more than the staged blocks plus the tail's own 16
        assert reach == 64 * loop_nb + (16 if tail_bytes else 0), L
        if not tail:
            seen_plain += 1
            continue
        seen_tail += 1
        seen_len_only += u < 0
        # words 0..3: (data & keep) | mark must give the padded words for any data
        for k in range(4):
            assert (M32 & keep[k]) | mark[k] == ones[k], (L, k)
            assert (0 & keep[k]) | mark[k] == zeros[k], (L, k)
            assert keep[k] & mark[k] == 0, (L, k)
        # words 4..15 are padding only: 4 and 14 / 15 can be non-zero
        assert all(ones[k] == zeros[k] for k in range(4, 16)), L
        assert all(ones[k] == 0 for k in range(5, 14)), L
        c4, c14, c15 = ones[4], ones[14], ones[15]
        want = [(K4 + c4) & M32, (K14 + c14) & M32, (K15 + c15) & M32, c4, c14, c15, _ssig1(c14), _ssig1(c15),
                _ssig0(c4), _ssig0(c14), (_ssig0(c15) + c14) & M32]
        assert tw == want, (L, [hex(x) for x in tw], [hex(x) for x in want])
    # Lengths 0..600 at three strides that suit every length (25 of every 64
    # lengths take the tail form, 8 of them with a length-only final block):
    # both forms were seen.
    assert seen_tail >= 700 and seen_plain >= 1000 and seen_len_only >= 200, (seen_tail, seen_plain, seen_len_only)


def test_stride_rules(rows):
    by = {(r[0], r[1]): r[2] for r in rows}
    assert by[(272, 272)] == 1 and by[(55, 55)] == 0 and by[(55, 4096)] == 1
    assert by[(100, 6)] == 0 and by[(100, 0)] == 1
    assert by[(100, 1 << 32)] == 0 and by[(100, (1 << 32) - 4)] == 1
