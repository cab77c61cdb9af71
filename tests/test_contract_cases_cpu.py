"""The cases of tests/contract_cases.py hold every class that
tests/test_gpu_device_contracts.py relies on, cannot touch memory outside their
allocations whatever a loader does, agree with plain hashlib where they are in
range, and bite: under each of three wrong models of a loader exactly the
predicted lists and messages get another digest.  So the GPU tests fail on a
subtly wrong kernel, and no kernel has to be broken to show it.  No GPU needed."""
import hashlib
import os
import re

import numpy as np
import pytest

import contract_cases as cc
import oracle_py

HASHERS = ("sha256", "sha512_256")
KERNELS_H = os.path.join(oracle_py.ROOT, "mirbft_amd", "csrc", "mirsha_kernels.h")
MIRSHA_H = os.path.join(oracle_py.ROOT, "include", "mirsha.h")
WRAPPING = {1 << 27, (1 << 27) + 5, (1 << 27) + 76, (1 << 28) + 1, 1 << 31, (1 << 31) + 3}


def differing(a, b):
    return set(np.flatnonzero((a != b).any(axis=1)).tolist())


# ---- constants and the header's sentences ---------------------------------------
def test_constants_equal_the_headers():
    text = open(KERNELS_H).read()
    m = re.search(r"constexpr\s+uint32_t\s+kMaxListDigests\s*=\s*\(1u\s*<<\s*27\)\s*-\s*1u\s*;", text)
    assert m and cc.K_MAX_LIST_DIGESTS == (1 << 27) - 1
    m = re.search(r"constexpr\s+uint64_t\s+kMaxBufferArena\s*=\s*(0x[0-9a-fA-F]+)ull\s*;", text)
    assert m and int(m.group(1), 16) == cc.K_MAX_BUFFER_ARENA
    m = re.search(r"constexpr\s+uint32_t\s+kNullIndex\s*=\s*(0x[0-9a-fA-F]+)u?\s*;", text)
    assert m and int(m.group(1), 16) == cc.NULL == oracle_py.NULL
    api = open(MIRSHA_H).read()
    assert re.search(r"#define\s+MIRSHA_MAX_DEVICE_ARENA_BYTES\s+0xFFFFFF00u", api)
    assert re.search(r"#define\s+MIRSHA_NULL_INDEX\s+0xFFFFFFFFu", api)


def test_the_header_states_the_models():
    api = " ".join(open(MIRSHA_H).read().replace("*", " ").split())
    assert "reads at or past arena_len rounded up to a multiple of 4 return 0" in api
    assert "up to 3 bytes behind arena_len must be readable" in api
    assert "off + len must stay below 2^32" in api
    assert "every index in [n_digests, MIRSHA_NULL_INDEX), whatever its value, contributes 32 zero bytes" in api


# ---- lists -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def tab():
    return cc.table()


def test_table_and_values(tab):
    assert tab.shape == (cc.N_ROWS, 32) == (85, 32) and cc.N_DIGESTS == 77 and tab.min() >= 1
    assert len({r.tobytes() for r in tab}) == cc.N_ROWS
    assert cc.CONTROLS == (0, 76) and all(v < cc.N_DIGESTS for v in cc.CONTROLS)
    assert cc.OUT_OF_RANGE == (77, 78, 84, 2**27 - 1, 2**27, 2**27 + 5, 2**27 + 76, 2**28 + 1, 2**31, 2**31 + 3,
                               0xFFFFFFFE)
    assert all(cc.N_DIGESTS <= v < cc.NULL for v in cc.OUT_OF_RANGE)
    assert len(cc.SHAPES) == 8
    for v in (0, 77, 1 << 31):
        assert [make(v) for make in cc.SHAPES.values()] == [
            [v], [5, v], [v, 5], [1, 2, 3, v], [1, 2, 3, 4, v], [cc.NULL, v, 5], [v, cc.NULL], [v] * 5]


def test_list_census():
    no_null, nulls = cc.list_launch("no_null"), cc.list_launch("nulls")
    names = {n for n, _ in no_null}
    for v in cc.CONTROLS + cc.OUT_OF_RANGE:
        for s in cc.SHAPES:
            assert ((v, s) in names) == (s not in cc.NULL_SHAPES), (v, s)
    assert not any(cc.NULL in ids for _, ids in no_null), "one NULL and the optimistic pass is not alone"
    names = {n for n, _ in nulls}
    for v in cc.CONTROLS + cc.OUT_OF_RANGE + (cc.NULL,):
        for s in cc.SHAPES:
            assert (v, s) in names, (v, s)
    for launch in (no_null, nulls):
        assert len(launch) > 64, "two waves at least"
        assert len({n for n, _ in launch}) == len(launch)
        for w in range(0, len(launch), 64):
            wave = launch[w:w + 64]
            # all-in-range lists sit beside the cases in every wave
            assert any(all(i < cc.N_DIGESTS for i in ids) and ids for _, ids in wave)
            assert any(any(cc.N_DIGESTS <= i < cc.NULL for i in ids) for _, ids in wave)
            # every wave of the second launch compacts
            assert any(cc.NULL in ids for _, ids in wave) == (launch is nulls)
    singles = cc.single_list_launches()
    assert [l[0][1] for l in singles] == [[5, v] for v in cc.OUT_OF_RANGE] and all(len(l) == 1 for l in singles)
    assert [ids for _, ids in cc.empty_table_launch()] == [[0], [5, cc.NULL], []]
    big = cc.tiled(nulls, 64 * 256 + 1)
    assert len(big) == 64 * 256 + 1 and big[len(nulls)] == nulls[0] and big[-1] == nulls[(64 * 256) % len(nulls)]
    idx, first = cc.flatten(nulls)
    assert first[0] == 0 and first[-1] == idx.size and first.size == len(nulls) + 1
    assert idx[first[3]:first[4]].tolist() == nulls[3][1]


def test_lists_cannot_leave_the_table():
    """A loader with no range check reads the row an index names, so every index
    that names one names it inside the allocation: below 2^27 that is the index
    itself, from 2^27 on its 32-bit offset.  2^27 - 1 and 0xFFFFFFFE excepted:
    their offsets are the last 64 bytes of the 32-bit range, which only a
    descriptor over a 4 GiB table admits; every read here goes through the
    hardware's check of a descriptor of 77 rows (or none)."""
    used = {i for kind in ("no_null", "nulls") for _, ids in cc.list_launch(kind) for i in ids}
    used |= {i for l in cc.single_list_launches() for _, ids in l for i in ids}
    assert set(cc.OUT_OF_RANGE) | set(cc.CONTROLS) | {cc.NULL} <= used
    assert cc.N_DIGESTS <= min(cc.SLACK_ROWS) and max(cc.SLACK_ROWS) == cc.N_ROWS - 1
    for i in used - {cc.NULL}:
        o = (32 * i) & 0xFFFFFFFF
        if i < 1 << 27:
            assert i < cc.N_ROWS or i == cc.K_MAX_LIST_DIGESTS, i
        assert o + 32 <= 32 * cc.N_ROWS or o >= (1 << 32) - 64, i
    assert 32 * cc.K_MAX_LIST_DIGESTS == 0xFFFFFFE0


@pytest.mark.parametrize("hasher", HASHERS)
def test_list_controls_are_plain_hashlib(tab, hasher):
    for kind in ("no_null", "nulls"):
        lists = cc.list_launch(kind)
        want = cc.want_lists(hasher, tab, cc.N_DIGESTS, lists)
        seen = 0
        for (name, ids), got in zip(lists, want):
            if all(i < cc.N_DIGESTS or i == cc.NULL for i in ids):
                seen += 1
                plain = hashlib.new(hasher, b"".join(tab[i].tobytes() for i in ids if i != cc.NULL)).digest()
                assert got.tobytes() == plain, name
        assert seen >= 10 + 2 * 6
    # the model by hand: a slack row is zeros, not the bytes that lie there
    one = cc.want_lists(hasher, tab, cc.N_DIGESTS, [(None, [5, 84])])[0].tobytes()
    assert one == hashlib.new(hasher, tab[5].tobytes() + bytes(32)).digest()
    assert one != hashlib.new(hasher, tab[5].tobytes() + tab[84].tobytes()).digest()
    empty = cc.want_lists(hasher, tab, 0, cc.empty_table_launch())
    z = hashlib.new(hasher, bytes(32)).digest()
    assert [r.tobytes() for r in empty] == [z, z, hashlib.new(hasher, b"").digest()]


@pytest.mark.parametrize("hasher", HASHERS)
def test_lists_bite_on_a_wrapping_row_offset(tab, hasher):
    """Wrong model 1: (32 id) mod 2^32 checked against 32 n_digests.  Exactly the
    lists that hold 2^27, 2^27 + 5, 2^27 + 76, 2^28 + 1, 2^31 or 2^31 + 3 differ;
    77, 78, 84, 2^27 - 1 and 0xFFFFFFFE do not wrap onto a row."""
    assert {v for v in cc.OUT_OF_RANGE if cc.wraps([v])} == WRAPPING
    launches = [cc.list_launch("no_null"), cc.list_launch("nulls")] + cc.single_list_launches()
    total = 0
    for lists in launches:
        want = cc.want_lists(hasher, tab, cc.N_DIGESTS, lists)
        wrong = cc.want_lists(hasher, tab, cc.N_DIGESTS, lists, cc.row_wrapping)
        predicted = {k for k, (_, ids) in enumerate(lists) if cc.wraps(ids)}
        assert predicted == {k for k, (n, _) in enumerate(lists) if n[0] in WRAPPING}
        assert differing(want, wrong) == predicted
        total += len(predicted)
    assert total == 6 * 6 + 6 * 8 + 6
    # and a loader with no range check at all gets every slack row wrong too
    raw = lambda t, n, i: t[((32 * i) & 0xFFFFFFFF) // 32].tobytes() if (32 * i) & 0xFFFFFFFF < 32 * cc.N_ROWS else bytes(32)
    lists = cc.list_launch("nulls")
    got = differing(cc.want_lists(hasher, tab, cc.N_DIGESTS, lists), cc.want_lists(hasher, tab, cc.N_DIGESTS, lists, raw))
    assert got == {k for k, (n, _) in enumerate(lists) if n[0] in WRAPPING | set(cc.SLACK_ROWS)}


# ---- arenas ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def alloc():
    return cc.nonzero_bytes(np.random.default_rng([7, 6]), cc.ARENA_ALLOC)


def test_arena_census():
    assert cc.ARENA_ALLOC == 4096 and cc.ARENA_LENS == (1000, 1001, 1002, 1003)
    assert set(cc.INSIDE) >= {0, 1, 5, 64, 130}
    assert cc.OVERHANG == (1, 2, 3, 4, 5, 17, 63, 64, 65, 127, 128, 129, 200)
    assert cc.PAST == (0, 1, 7, 300) and cc.PAST_LENS == (0, 1, 55, 56, 111, 112, 200)
    for A in cc.ARENA_LENS:
        msgs = cc.overhang_messages(A)
        cls = {c: (o, n) for c, o, n in msgs}
        assert len(cls) == len(msgs) > 64, "two groups at least"
        for k in cc.INSIDE:
            for h in cc.OVERHANG:
                assert cls[("partial", k, h)] == (A - k, k + h)
        for h in cc.OVERHANG:  # every overhang at every byte alignment under this residue
            assert {(A - k) % 4 for k in cc.INSIDE} == {0, 1, 2, 3}
        for d in cc.PAST:
            for L in cc.PAST_LENS:
                assert cls[("past", d, L)] == (A + d, L)
        controls = [(o, n) for c, o, n in msgs if c[0] == "control"]
        assert len(controls) == len(cc.CONTROL_MSGS) and all(o >= 0 and o + n <= A for o, n in controls)
        assert sum(o + n == A and n > 0 for o, n in controls) == 2, "controls that end exactly at arena_len"
        for w in range(0, len(msgs), 64):  # a wave mixes the classes
            assert {c[0] for c, _, _ in msgs[w:w + 64]} == {"partial", "past", "control"}
    assert {A % 4 for A in cc.ARENA_LENS} == {0, 1, 2, 3}
    tile = cc.tile_messages()
    assert len(tile) == 64 and all(n == 272 and o % 4 == 0 and o == 272 * i for i, (_, o, n) in enumerate(tile))
    for A in cc.TILE_ARENA_LENS:
        over = [i for i, (_, o, n) in enumerate(tile) if o + n > A]
        assert over == [62, 63] and tile[62][1] < A < tile[62][1] + 272 and tile[63][1] >= cc.rounded(A)
    assert {A % 4 for A in cc.TILE_ARENA_LENS} == {0, 1, 2, 3}


def test_top_census():
    assert cc.TOP_ALLOC == cc.K_MAX_BUFFER_ARENA + 8192
    assert cc.WINDOWS == ((0, 65536), (2**31 - 4096, 2**31 + 4096), (cc.K_MAX_BUFFER_ARENA - 65536, cc.TOP_ALLOC))
    w = cc.Windows()
    assert all(p.min() >= 1 for _, p in w.parts)
    for A in (cc.K_MAX_BUFFER_ARENA, cc.K_MAX_BUFFER_ARENA + 1, cc.K_MAX_BUFFER_ARENA + 4):
        msgs = cc.top_messages(A)
        assert 125 <= len(msgs) <= 135 and max(n for _, _, n in msgs) == 5000
        assert sorted(n for _, _, n in msgs)[-2] <= 700
        by = {k: [(o, n) for c, o, n in msgs if c[0] == k] for k in ("start", "mid", "top")}
        assert min(o for o, _ in by["start"]) == 3, "a lead of 3 bytes"
        assert all(o < cc.MID < o + n for o, n in by["mid"]) and (cc.MID - 2501, 5000) in by["mid"]
        assert msgs[-1][1] + msgs[-1][2] == A and msgs[-1][2] > 0, "the last message ends exactly at arena_len"
        assert all(o + n <= A for _, o, n in msgs)
        for part in by.values():
            assert {o % 4 for o, _ in part} == {0, 1, 2, 3}
        for _, o, n in msgs:
            assert len(w.read(o, o + n)) == n  # inside a filled window
    # group b's cases at the top: arena_len of every residue, the overhang inside the slack and below 2^32
    assert {A % 4 for A in range(cc.K_MAX_BUFFER_ARENA - 3, cc.K_MAX_BUFFER_ARENA + 1)} == {0, 1, 2, 3}
    for A in range(cc.K_MAX_BUFFER_ARENA - 3, cc.K_MAX_BUFFER_ARENA + 1):
        msgs = cc.overhang_messages(A, end_below=1 << 32)
        cls = {c for c, _, _ in msgs}
        assert {("partial", k, h) for k in cc.INSIDE for h in cc.OVERHANG} <= cls
        assert {("past", d, L) for d in (0, 1, 7) for L in cc.PAST_LENS} <= cls
        assert not any(c[:2] == ("past", 300) for c in cls), "off itself would lie past 2^32"
        for _, o, n in msgs:
            assert o + n < 1 << 32 and len(w.read(o, o + n)) == n


def test_messages_cannot_leave_their_allocation():
    for A in cc.ARENA_LENS:
        assert all(o >= 0 and o + n + cc.SLACK <= cc.ARENA_ALLOC for _, o, n in cc.overhang_messages(A))
    assert all(o + n + cc.SLACK <= cc.TILE_ALLOC for _, o, n in cc.tile_messages())
    for A in (cc.K_MAX_BUFFER_ARENA, cc.K_MAX_BUFFER_ARENA + 1, cc.K_MAX_BUFFER_ARENA + 4):
        assert all(o >= 0 and o + n + cc.SLACK <= cc.TOP_ALLOC for _, o, n in cc.top_messages(A))
    for A in range(cc.K_MAX_BUFFER_ARENA - 3, cc.K_MAX_BUFFER_ARENA + 1):
        assert all(o + n + cc.SLACK <= cc.TOP_ALLOC for _, o, n in cc.overhang_messages(A, end_below=1 << 32))


def launches(alloc):
    """(read, arena_len, messages) of every small-arena launch."""
    out = [(cc.reader(alloc), A, cc.overhang_messages(A)) for A in cc.ARENA_LENS]
    tile = cc.nonzero_bytes(np.random.default_rng([7, 7]), cc.TILE_ALLOC)
    out += [(cc.reader(tile), A, cc.tile_messages()) for A in cc.TILE_ARENA_LENS]
    w = cc.Windows()
    out += [(w.read, A, cc.overhang_messages(A, end_below=1 << 32))
            for A in range(cc.K_MAX_BUFFER_ARENA - 3, cc.K_MAX_BUFFER_ARENA + 1)]
    return out


@pytest.mark.parametrize("hasher", HASHERS)
def test_arena_controls_are_plain_hashlib(alloc, hasher):
    for read, A, msgs in launches(alloc):
        want = cc.want_arena(hasher, read, cc.rounded(A), msgs)
        seen = 0
        for (c, o, n), got in zip(msgs, want):
            if o + n <= A:
                seen += 1
                assert got.tobytes() == hashlib.new(hasher, read(o, o + n)).digest(), (A, c)
        assert seen >= 18
    w = cc.Windows()
    for A in (cc.K_MAX_BUFFER_ARENA, cc.K_MAX_BUFFER_ARENA + 1, cc.K_MAX_BUFFER_ARENA + 4):
        msgs = cc.top_messages(A)
        want = cc.want_arena(hasher, w.read, cc.rounded(A), msgs)
        assert [r.tobytes() for r in want] == [hashlib.new(hasher, w.read(o, o + n)).digest() for _, o, n in msgs]
    # the model by hand: arena_len 1001, bytes 1001..1003 are real, 1004 onward zero
    got = cc.want_arena(hasher, cc.reader(alloc), cc.rounded(1001), [(None, 996, 12)])[0].tobytes()
    assert got == hashlib.new(hasher, alloc[996:1004].tobytes() + bytes(4)).digest()


@pytest.mark.parametrize("hasher", HASHERS)
def test_arenas_bite_on_a_missing_and_on_a_strict_range_check(alloc, hasher):
    """Wrong model 2 reads the real bytes at and above R: every message with a
    byte there differs.  Wrong model 3 reads zeros from arena_len instead of R:
    every message with a byte in [arena_len, R) differs, none where arena_len
    is a multiple of 4."""
    for read, A, msgs in launches(alloc):
        R = cc.rounded(A)
        want = cc.want_arena(hasher, read, R, msgs)
        unchecked = cc.want_arena(hasher, read, 1 << 40, msgs)
        strict = cc.want_arena(hasher, read, A, msgs)
        p2 = {k for k, (_, o, n) in enumerate(msgs) if cc.reads_at_or_past(R, o, n)}
        p3 = {k for k, (_, o, n) in enumerate(msgs) if cc.reads_the_partial_word(A, o, n)}
        assert differing(want, unchecked) == p2 and differing(want, strict) == p3
        assert (len(p3) == 0) == (A % 4 == 0)
        named = {c for c, _, _ in msgs}
        if ("partial", 0, 1) in named:
            k = [c for c, _, _ in msgs].index(("partial", 5, 4))
            assert k in p2 and (k in p3) == (A % 4 != 0)
            # an overhang that ends inside the partial word is all real: only the strict model misses it
            k = [c for c, _, _ in msgs].index(("partial", 1, 1))
            assert (k in p2) == (A % 4 == 0) and (k in p3) == (A % 4 != 0)
            # every overhang of 4 or more crosses R; every overhang holds the byte at arena_len
            assert len(p2) >= 6 * 10 and (A % 4 == 0 or len(p3) >= 6 * 13)
        else:
            assert p2 == {62, 63} and p3 == ({62} if A % 4 else set())
