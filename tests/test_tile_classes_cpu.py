"""The tile-class stream of tests/tileclasses.py keeps every class of
hash_tile's classification (far / aligned / uni / tail_ok) for every
arena_len % 4, so tests/test_gpu_tile_classes.py cannot silently lose a class
when the generator is edited.  No GPU needed."""
import hashlib

import numpy as np
import pytest

import oracle_py
import tileclasses as tc


@pytest.fixture(scope="module", params=[0, 1, 2, 3], ids=lambda m: f"tail{m}")
def stream(request):
    arena, off, lens, meta = tc.build(request.param, seed=0)
    return request.param, arena, off, lens, meta, tc.classify(off, lens, arena.size)


def test_shape_and_bounds(stream):
    tail_mod, arena, off, lens, meta, _ = stream
    assert arena.size % 16 == tail_mod
    assert len(meta) == len(tc.LENGTHS) * len(tc.ALIGNMENTS) * len(tc.PLACEMENTS) == 192
    assert len(set(meta)) == len(meta)
    assert off.size == lens.size == 64 * len(meta)
    assert (off.astype(np.int64) >= 0).all()
    assert (off.astype(np.int64) + lens <= arena.size).all()
    assert arena.size < 1 << 20


def test_deterministic():
    a = tc.build(2, seed=5)
    b = tc.build(2, seed=5)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    assert not np.array_equal(a[0], tc.build(2, seed=6)[0])


def test_placement_decides_far(stream):
    _, arena, off, lens, meta, cls = stream
    for t, (_, al, pl) in enumerate(meta):
        assert cls["far"][t] == (pl == "body"), meta[t]
        o, L = off[64 * t:64 * t + 64].astype(np.int64), lens[64 * t:64 * t + 64]
        if pl == "body":
            assert (o + L).max() <= arena.size - tc.BODY_MARGIN
        else:  # the last message ends at the arena end, or as near below it as its alignment allows
            assert arena.size - (16 if al == "a16" else 4) < int((o + L).max()) <= arena.size, meta[t]


def test_alignment_rules(stream):
    _, _, off, lens, meta, cls = stream
    for t, (ln, al, _) in enumerate(meta):
        o = off[64 * t:64 * t + 64].astype(np.int64)
        if al == "a16":
            assert (o % 16 == 0).all()
        elif al in ("a4", "r1", "r3"):
            assert (o % 4 == {"a4": 0, "r1": 1, "r3": 3}[al]).all()
        elif al == "packed":
            assert o[0] % 4 == 0 and np.array_equal(o[1:], o[:-1] + lens[64 * t:64 * t + 63])
        assert cls["aligned"][t] == bool((o % 4 == 0).all())
        if al in ("a16", "a4"):
            assert cls["aligned"][t]
        if al in ("r1", "r3"):
            assert not cls["aligned"][t]


def test_single_lane_tiles_hang_on_one_lane(stream):
    """lane0 / lane63 / lane31 tiles: not aligned, and aligned without that lane."""
    _, arena, off, lens, meta, cls = stream
    seen = 0
    for t, (_, al, _) in enumerate(meta):
        if al not in tc.SINGLE_LANE:
            continue
        seen += 1
        lane, shift = tc.SINGLE_LANE[al]
        o = off[64 * t:64 * t + 64].astype(np.int64)
        assert not cls["aligned"][t]
        assert o[lane] % 4 == shift
        keep = np.arange(64) != lane
        assert (o[keep] % 4 == 0).all()
        rest = tc.classify(o[keep], lens[64 * t:64 * t + 64][keep], arena.size)
        assert rest["aligned"][0]
    assert seen == 3 * len(tc.LENGTHS) * len(tc.PLACEMENTS)


def test_length_recipes_classify_as_named(stream):
    _, _, _, lens, meta, cls = stream
    for t, (ln, _, _) in enumerate(meta):
        L = lens[64 * t:64 * t + 64]
        if ln[0] == "u":
            assert cls["uni"][t] and (L == int(ln[1:])).all()
            assert cls["tail_ok"][t] == (ln in ("u144", "u128", "u60", "u0")), ln
        else:
            assert not cls["uni"][t] and not cls["tail_ok"][t]
            assert cls["one_nb"][t] == (ln in ("one_nb", "one_nb_x4")), ln
        if ln == "one_nb_x4":
            assert (L % 4 == 0).all() and L.min() >= 56 and L.max() <= 119
        if ln == "one_long":
            assert sorted(L)[-2:] == [20, 700] and cls["wave_nb"][t] == 12


def test_all_16_cells_populated(stream):
    _, _, _, _, _, cls = stream
    census = tc.census(cls)
    assert len(census) == 16 and sum(census.values()) == 192
    assert min(census.values()) >= 4, census
    # aligned and mixed, the class the random streams never compose, near and far
    for far in (True, False):
        assert census[(far, True, "mixed_one_nb")] >= 4 and census[(far, True, "mixed_nb")] >= 4


def test_partial_tile_helper(stream):
    _, arena, off, lens, meta, _ = stream
    k = tc.tile_index(meta, "one_nb_x4", "lane31", "body")
    o, L = tc.with_partial_tile(off, lens, k, 63)
    assert o.size == 64 * k + 63 and np.array_equal(o, off[:o.size]) and np.array_equal(L, lens[:o.size])
    cls = tc.classify(o, L, arena.size)
    assert not cls["aligned"][k]
    o, L = tc.with_partial_tile(off, lens, k, 1)  # lane 31 is idle now
    assert tc.classify(o, L, arena.size)["aligned"][k]


def test_oracle_and_hashlib_agree(stream):
    _, arena, off, lens, _, _ = stream
    raw = arena.tobytes()
    want = np.frombuffer(b"".join(hashlib.sha256(raw[int(o):int(o) + int(n)]).digest() for o, n in zip(off, lens)),
                         dtype=np.uint8).reshape(-1, 32)
    assert np.array_equal(oracle_py.hash_requests(arena, off, lens), want)
