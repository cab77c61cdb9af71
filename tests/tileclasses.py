"""A deterministic request stream with one 64-message tile per class of
hash_tile's tile classification (mirbft_amd/csrc/mirsha_kernels.hip), and that
classification restated in Python.  Test infrastructure.

hash_tile decides per tile, with wave-wide predicates over its valid lanes:

  far      every lane has off + 64 * wave_nb + 20 <= records, with
           records = (arena_len + 3) & ~3 and wave_nb the block count of the
           tile's longest message: plain loads (else range-checked chunks)
  aligned  every lane has off % 4 == 0: 4 loads per block, and with `far` the
           LDS-DMA / pipelined block loops
  uni      every lane has the same length: padding once after the transpose
  tail_ok  uni and at most 16 message bytes in the final block: tail rounds

build() crosses 12 length recipes x 8 start alignments x 2 placements into 192
whole tiles (12,288 messages) in launch order, so with d_order = None the test,
not the host's bucketing, decides what a tile is made of.
"""
import numpy as np

LENGTHS = ("u144", "u128", "u60", "u100", "u93", "u0", "one_nb", "one_nb_x4", "mixed_nb", "pad_edges", "one_long",
           "zeros_mixed")
ALIGNMENTS = ("a16", "a4", "r1", "r3", "packed", "lane0", "lane63", "lane31")
PLACEMENTS = ("body", "end")
# alignment -> (lane, byte shift) of the one lane that is not 4-byte aligned
SINGLE_LANE = {"lane0": (0, 1), "lane63": (63, 2), "lane31": (31, 3)}
# Body tiles stay this far from the arena end: past any lane's reach (the
# longest message here is 700 bytes: 64 * 12 + 20 bytes from a lane's start).
BODY_MARGIN = 2048
CELLS = [(far, al, kind) for far in (True, False) for al in (True, False)
         for kind in ("uni_tail", "uni", "mixed_one_nb", "mixed_nb")]


def blocks_for_len(L):
    """SHA-256 blocks of an L-byte message (sha256_device.h)."""
    return (np.asarray(L, dtype=np.int64) + 72) >> 6


def _lengths(name, rng):
    if name[0] == "u":
        return np.full(64, int(name[1:]), dtype=np.int64)
    if name == "one_nb":  # 56..119: two blocks each
        return rng.integers(56, 120, 64)
    if name == "one_nb_x4":
        return 4 * rng.integers(14, 30, 64)
    if name == "mixed_nb":
        return rng.integers(0, 330, 64)
    if name == "pad_edges":
        return np.array([55, 56, 57, 63, 64, 65, 119, 120] * 8, dtype=np.int64)
    if name == "one_long":  # wave_nb far above most lanes' block count
        ln = np.full(64, 20, dtype=np.int64)
        ln[int(rng.integers(0, 64))] = 700
        return ln
    assert name == "zeros_mixed"
    ln = rng.integers(1, 200, 64)
    ln[::2] = 0
    return ln


def _rule(align, lane):
    """(modulus, residue) of lane's start offset; None = byte-packed."""
    if align == "a16":
        return 16, 0
    if align in ("a4", "r1", "r3"):
        return 4, {"a4": 0, "r1": 1, "r3": 3}[align]
    if align == "packed":
        return (4, 0) if lane == 0 else None  # the tile's base is aligned, the rest follows the lengths
    k, d = SINGLE_LANE[align]
    return 4, (d if lane == k else 0)


def _place_forward(lens, align, pos):
    off = []
    for i, L in enumerate(lens.tolist()):  # plain ints: these loops are the cost of build()
        r = _rule(align, i)
        if r is not None:
            pos += (r[1] - pos) % r[0]
        off.append(pos)
        pos += L
    return np.array(off, dtype=np.int64), pos


def _place_backward(lens, align, end):
    """Lane 63's message ends at `end`, or as few bytes below it as its rule allows."""
    if align == "packed":  # back to back below `end`, the base rounded down to 4 bytes
        base = (end - int(lens.sum())) & ~3
        return _place_forward(lens, align, base)[0]
    off = []
    for i, L in zip(range(63, -1, -1), lens.tolist()[::-1]):
        m, res = _rule(align, i)
        end -= L
        end -= (end - res) % m
        off.append(end)
    return np.array(off[::-1], dtype=np.int64)


def build(tail_mod, seed=0):
    """(arena, off, lens, meta): meta[t] = (lengths, alignment, placement) of tile t.
    arena_len = a multiple of 16 + tail_mod."""
    assert 0 <= tail_mod < 4
    rng = np.random.default_rng([seed, 77])
    tiles = [(ln, al, pl) for ln in LENGTHS for al in ALIGNMENTS for pl in PLACEMENTS]
    lens = [_lengths(ln, rng) for ln, _, _ in tiles]
    offs = [None] * len(tiles)
    pos = 0
    for t, (_, al, pl) in enumerate(tiles):
        if pl == "body":
            offs[t], pos = _place_forward(lens[t], al, pos)
    arena_len = ((pos + BODY_MARGIN + 15) & ~15) + 16 + tail_mod
    for t, (_, al, pl) in enumerate(tiles):
        if pl == "end":
            offs[t] = _place_backward(lens[t], al, arena_len)
    arena = np.random.default_rng([seed, 78]).integers(0, 256, arena_len, dtype=np.uint8)
    off = np.concatenate(offs).astype(np.uint64)
    return arena, off, np.concatenate(lens).astype(np.uint32), tiles


def classify(off, lens, arena_len):
    """hash_tile's predicates per tile of 64 (the last one may be partial):
    dict of bool arrays far / aligned / uni / tail_ok / one_nb, and wave_nb."""
    off = np.asarray(off, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    records = (int(arena_len) + 3) & ~3
    n_tiles = (off.size + 63) // 64
    valid = (np.arange(64 * n_tiles) < off.size).reshape(n_tiles, 64)
    o = np.zeros(64 * n_tiles, dtype=np.int64)
    L = np.zeros(64 * n_tiles, dtype=np.int64)
    o[:off.size], L[:off.size] = off, lens
    o, L = o.reshape(n_tiles, 64), L.reshape(n_tiles, 64)
    max_l = np.where(valid, L, 0).max(axis=1)
    min_l = np.where(valid, L, 1 << 32).min(axis=1)
    wave_nb = blocks_for_len(max_l)
    uni = max_l == min_l
    return {"wave_nb": wave_nb,
            "far": (~valid | (o + 64 * wave_nb[:, None] + 20 <= records)).all(axis=1),
            "aligned": (~valid | (o % 4 == 0)).all(axis=1),
            "uni": uni,
            "tail_ok": uni & (min_l - 64 * (wave_nb - 1) <= 16),
            "one_nb": (~valid | (blocks_for_len(L) == wave_nb[:, None])).all(axis=1)}


def cells(cls):
    """Per tile its cell (far, aligned, kind) of CELLS."""
    kind = np.where(cls["tail_ok"], "uni_tail",
                    np.where(cls["uni"], "uni", np.where(cls["one_nb"], "mixed_one_nb", "mixed_nb")))
    return [(bool(f), bool(a), str(k)) for f, a, k in zip(cls["far"], cls["aligned"], kind)]


def census(cls):
    """Tile count per cell of CELLS."""
    got = cells(cls)
    return {c: got.count(c) for c in CELLS}


def with_partial_tile(off, lens, tile, r):
    """The stream's first `tile` tiles, then the first r messages of tile `tile`
    as a partial last tile (idle lanes read entry n - 1)."""
    n = 64 * tile + r
    return off[:n].copy(), lens[:n].copy()


def tile_index(meta, lengths, alignment, placement):
    return meta.index((lengths, alignment, placement))
