"""The list-class stream of tests/listclasses.py keeps every class of the
dependent pass's wave-wide decisions populated, restates the header's
thresholds correctly, and has two independent references that agree, so
tests/test_gpu_list_classes.py cannot silently lose a class or be routed to
another kernel when the generator or a threshold is edited.  No GPU needed."""
import hashlib
import os
import re

import numpy as np
import pytest

import listclasses as lc
import oracle_py

HEADER = os.path.join(oracle_py.ROOT, "mirbft_amd", "csrc", "mirsha_kernels.h")
EMPTY = np.frombuffer(hashlib.sha256(b"").digest(), dtype=np.uint8)


@pytest.fixture(scope="module")
def stream():
    idx, first, n_digests, meta = lc.build(seed=0)
    return idx, first, n_digests, meta, lc.classify(idx, first)


def _group(stream, name):
    idx, first, _, meta, _ = stream
    g = lc.group_index(meta, *name)
    f = first[64 * g:64 * g + 65].astype(np.int64)
    return g, [idx[f[i]:f[i + 1]] for i in range(64)]


def test_shape_and_bounds(stream):
    idx, first, n_digests, meta, cls = stream
    assert len(meta) == len(lc.COUNTS) * len(lc.NULLS) * len(lc.INDICES) == 273
    assert len(set(meta)) == len(meta)
    assert first.size == 64 * len(meta) + 1 and first[0] == 0 and first[-1] == idx.size
    assert (np.diff(first.astype(np.int64)) >= 0).all()
    assert first[-1] > first[-2], "the last list must be non-empty: the descriptor ends behind its last entry"
    assert n_digests == lc.N_DIGESTS == 1024
    live = idx[idx != lc.K_NULL_INDEX]
    assert live.max() == n_digests - 1 and live.min() == 0
    assert len(meta) <= lc.K_PAIR_MAX_GROUPS, "as composed the stream is a pair-kernel plan"
    assert cls["wave_nb"].size == len(meta)


def test_deterministic():
    a, b = lc.build(seed=5), lc.build(seed=5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    assert not np.array_equal(a[0], lc.build(seed=6)[0])


def test_thresholds_equal_the_header():
    text = open(HEADER).read()

    def const(name):
        m = re.search(r"constexpr\s+uint32_t\s+" + name + r"\s*=\s*(0[xX][0-9a-fA-F]+|\d+)u?\s*;", text)
        assert m, f"{name} not found in mirsha_kernels.h"
        return int(m.group(1), 0)

    assert const("kPairMaxGroups") == lc.K_PAIR_MAX_GROUPS
    assert const("kFusedChunkBlocks") == lc.K_FUSED_CHUNK_BLOCKS
    assert const("kNullIndex") == lc.K_NULL_INDEX == oracle_py.NULL


def test_count_recipes(stream):
    idx, first, _, meta, cls = stream
    raw = np.diff(first.astype(np.int64)).reshape(-1, 64)
    for g, (c, _, _) in enumerate(meta):
        if c[0] == "u":
            assert (raw[g] == int(c[1:])).all()
            assert cls["raw_shape"][g] == ("uni_even" if int(c[1:]) % 2 == 0 else "uni_odd")
        elif c == "edges":
            assert np.array_equal(raw[g], np.arange(64) % 10)
        elif c == "one_long":
            assert sorted(raw[g].tolist())[-2:] == [2, lc.ONE_LONG] and cls["raw_wave_nb"][g] == 21
        elif c == "zeros_mixed":
            assert (raw[g][::2] == 0).all() and raw[g][1::2].min() >= 1 and raw[g][1::2].max() <= 30
        elif c == "one_nb":
            assert set(raw[g].tolist()) == {2, 3} and cls["raw_shape"][g] == "mixed_one_nb"
        else:
            assert c == "mixed" and raw[g].max() <= 44 and cls["raw_shape"][g] == "mixed_nb"


def test_null_recipes(stream):
    idx, first, _, meta, cls = stream
    prefetched = set()
    for g, name in enumerate(meta):
        _, lists = _group(stream, name)
        nulls = [np.flatnonzero(v == lc.K_NULL_INDEX) for v in lists]
        lanes = [i for i in range(64) if nulls[i].size]
        nl = name[1]
        if nl == "none":
            assert lanes == []
        elif nl == "lane0_first":
            assert lanes == ([0] if lists[0].size else []) and nulls[0].tolist() == [0][:lists[0].size]
        elif nl == "lane63_last":
            assert lanes == ([63] if lists[63].size else [])
            assert nulls[63].tolist() == [lists[63].size - 1][:lists[63].size]
        elif nl == "lane31_all":
            assert lanes == ([31] if lists[31].size else []) and nulls[31].size == lists[31].size
        elif nl == "each_one":
            assert all(nulls[i].size == min(1, lists[i].size) for i in range(64))
            # found only as a prefetched entry wherever the list is long enough
            assert all(int(p[0]) >= 2 for p, v in zip(nulls, lists) if v.size > 2)
            prefetched |= {int(p[0]) for p in nulls if p.size}
            if name[0] in ("u8", "u9", "mixed"):
                assert set(lc.PREFETCHED) <= {int(p[0]) for p in nulls if p.size}, name
        elif nl == "all_null":
            assert all(nulls[i].size == lists[i].size for i in range(64))
            assert cls["shape"][g] == "uni_even" and cls["wave_nb"][g] == 1 and cls["has_empty"][g]
        else:
            assert nl == "half"
        assert cls["raw_nulls"][g] == ("none", "one_lane", "several_lanes")[min(len(lanes), 2)]
    assert set(lc.PREFETCHED) <= prefetched


def test_index_recipes(stream):
    _, _, n_digests, meta, _ = stream
    for name in meta:
        _, lists = _group(stream, name)
        if name[2] == "shared":
            for p in range(max(v.size for v in lists)):
                assert len({int(v[p]) for v in lists if v.size > p and v[p] != lc.K_NULL_INDEX}) <= 1, (name, p)
        elif name[2] == "edge":
            for v in lists:
                live = v[v != lc.K_NULL_INDEX]
                if live.size:
                    assert live[-1] == n_digests - 1 and (live.size == 1 or live[0] == 0)


def test_every_cell_populated(stream):
    cls = stream[4]
    raw = lc.raw_census(cls)
    assert len(raw) == 12 and sum(raw.values()) == 273
    assert min(raw.values()) >= 1, raw
    comp = lc.compacted_census(cls)
    assert set(comp) == set(lc.SHAPES) and sum(n for n, _ in comp.values()) == 273
    for shape, (groups, with_empty) in comp.items():
        # an empty list has the even count 0, so a group of one odd count cannot hold one
        assert groups >= 1 and (with_empty >= 1) == (shape != "uni_odd"), (shape, comp)
    # odd and even wave_nb both occur, so on one fused pair the ring slot parity carries over
    assert {int(v) % 2 for v in cls["wave_nb"]} == {0, 1}
    assert (cls["chunks"] == -(-cls["wave_nb"] // 2)).all() and cls["chunks"].min() == 1 and cls["chunks"].max() >= 11


def test_classify_by_hand():
    """Three lists (one partial group): [7, NULL], [NULL], [] over raw counts 2, 1, 0."""
    idx = np.array([7, lc.K_NULL_INDEX, lc.K_NULL_INDEX], dtype=np.uint32)
    first = np.array([0, 2, 3, 3], dtype=np.uint32)
    cls = lc.classify(idx, first)
    assert cls["raw_nulls"].tolist() == ["several_lanes"] and cls["raw_shape"].tolist() == ["mixed_nb"]
    assert cls["raw_wave_nb"].tolist() == [2]
    assert cls["shape"].tolist() == ["mixed_one_nb"] and cls["has_empty"].tolist() == [True]
    assert cls["wave_nb"].tolist() == [1] and cls["chunks"].tolist() == [1]
    assert lc.blocks_for_count([0, 1, 2, 3, 4, 5, 41]).tolist() == [1, 1, 2, 2, 3, 3, 21]


def test_partial_group_helper(stream):
    idx, first, _, meta, _ = stream
    tails = set()
    for name in lc.PARTIAL_GROUPS:
        g = lc.group_index(meta, *name)
        for r in (1, 63):
            ix, f = lc.with_partial_group(first, idx, g, r)
            assert f.size == 64 * g + r + 1 and f[-1] == ix.size
            assert np.array_equal(f, first[:f.size]) and np.array_equal(ix, idx[:ix.size])
            tails.add(int(f[-1] - f[-2]) % 4)
    assert tails == {0, 1, 2, 3}, "the descriptor's end must fall behind lists of every count mod 4"
    assert {"edges", "one_long"} <= {n[0] for n in lc.PARTIAL_GROUPS}
    assert {"each_one", "lane63_last"} <= {n[1] for n in lc.PARTIAL_GROUPS}
    # lane 63 is idle at r = 63, so its null no longer decides the ballot
    g = lc.group_index(meta, "u3", "lane63_last", "shared")
    assert lc.classify(idx, first)["raw_nulls"][g] == "one_lane"
    assert lc.classify(*lc.with_partial_group(first, idx, g, 63))["raw_nulls"][g] == "none"


def test_repeat_rotated(stream):
    idx, first, _, _, _ = stream
    n0 = first.size - 1
    for groups in (lc.K_PAIR_MAX_GROUPS, lc.K_PAIR_MAX_GROUPS + 1):
        ix, f, src = lc.repeat_rotated(idx, first, groups)
        assert f.size == 64 * groups + 1 and f[-1] == ix.size and src.size == 64 * groups
        assert np.array_equal(src[:n0], np.arange(n0)) and src[n0] == 29
        for k in (0, n0 - 1, n0, n0 + 1, 64 * groups - 1):
            s = int(src[k])
            assert np.array_equal(ix[f[k]:f[k + 1]], idx[first[s]:first[s + 1]])


def test_uniform_is_identity():
    idx, first = lc.uniform(11, 4)
    assert idx.tolist() == list(range(11)) and first.tolist() == [0, 4, 8, 11]


def test_oracle_and_hashlib_agree(stream):
    idx, first, n_digests, _, cls = stream
    dig = np.random.default_rng(3).integers(0, 256, (n_digests, 32), dtype=np.uint8)
    rows = [dig[i].tobytes() for i in range(n_digests)]
    want = np.empty((first.size - 1, 32), dtype=np.uint8)
    for k in range(first.size - 1):
        msg = b"".join(rows[i] for i in idx[first[k]:first[k + 1]].tolist() if i != lc.K_NULL_INDEX)
        want[k] = np.frombuffer(hashlib.sha256(msg).digest(), dtype=np.uint8)
    got = oracle_py.batch_digests(dig, idx, first)
    assert np.array_equal(got, want)
    # empty and all-null lists give the empty-message digest
    c = np.diff(first.astype(np.int64))
    nul = np.add.reduceat(np.concatenate([idx == lc.K_NULL_INDEX, [False]]), first[:-1].astype(np.int64)) * (c > 0)
    nothing = c == nul
    assert nothing.sum() > 64 * 3 * 8 and (got[nothing] == EMPTY).all() and not (got[~nothing] == EMPTY).all(axis=1).any()
