"""A deterministic stream of digest lists with one 64-list group per class of the
dependent pass's wave-wide decisions (mirbft_amd/csrc/mirsha_kernels.hip), and
those decisions restated in Python.  Test infrastructure.

Every form of the dependent pass gives one lane a list and decides per 64 lists:

  null ballot   sha256_lists_kernel hashes optimistically and, if __any lane met
                a null entry, compacts all 64 lists into scratch and hashes again
  wave_nb       wave_max of the lists' block counts (a list of c digests has
                (32 c + 72) >> 6 blocks): every lane loops that far and pads by
                `ordinal == c` on zero-filled, range-checked loads
                (list_block_words)
  pad_wave      sha256_chain_kernel<true>: __all lists full with an even count,
                then the final block runs from a constant schedule
  chunks        the fused producer waits per ceil(wave_nb / kFusedChunkBlocks)

build() crosses 13 count recipes x 7 null recipes x 3 index recipes into 273
whole groups (17,472 lists) over N_DIGESTS digests.  Where a recipe is vacuous
for a count (a null in an empty list) the group is emitted all the same.
"""
import numpy as np

from mirbft_amd import sharding

N_DIGESTS = 1024
# Restated from mirbft_amd/csrc/mirsha_kernels.h (tests/test_list_classes_cpu.py
# compares them with the header's text).
K_NULL_INDEX = 0xFFFFFFFF
K_PAIR_MAX_GROUPS = 512
K_FUSED_CHUNK_BLOCKS = 2

# u<c>: all 64 lists of c entries (marker parity, the padding-only block, the
# 4-digest chunk edge, the prefetch depths of indices and digests); one_nb: 2 or
# 3 entries, different counts with one block count (the raw view has no other
# source of that cell).
COUNTS = ("u0", "u1", "u2", "u3", "u4", "u5", "u8", "u9", "edges", "one_long", "mixed", "zeros_mixed", "one_nb")
NULLS = ("none", "lane0_first", "lane63_last", "lane31_all", "each_one", "half", "all_null")
INDICES = ("distinct", "edge", "shared")
ONE_LONG = 41
# each_one: one null per lane at a seeded position, at 2 or later where the list
# has more than two entries; the first lanes long enough get theirs at these
# positions, the entries ListBlocks (the list source of the lists, pair and
# chain kernels) holds prefetched in nx0 / nx1 and nn0 / nn1.
PREFETCHED = (2, 3, 4, 5)

RAW_NULLS = ("none", "one_lane", "several_lanes")
SHAPES = ("uni_even", "uni_odd", "mixed_one_nb", "mixed_nb")
RAW_CELLS = [(nl, sh) for nl in RAW_NULLS for sh in SHAPES]

# Groups behind which the GPU test cuts the stream to r = 1 and r = 63 lists of
# the group (with_partial_group): the descriptor of idx then ends behind a list
# of 0, 1, 2 and 3 entries (counts mod 4), inside a group whose ballot hangs on
# lane 0 (valid at every r) or on lane 63 (idle at every r < 64).
PARTIAL_GROUPS = (("edges", "none", "distinct"), ("one_long", "none", "edge"), ("u5", "each_one", "distinct"),
                  ("u3", "lane63_last", "shared"), ("u9", "lane0_first", "edge"), ("u2", "half", "shared"),
                  ("mixed", "lane63_last", "distinct"))


def blocks_for_count(c):
    """SHA-256 blocks of a list of c 32-byte digests (sha256_device.h)."""
    return (32 * np.asarray(c, dtype=np.int64) + 72) >> 6


def _counts(name, rng):
    if name[0] == "u":
        return np.full(64, int(name[1:]), dtype=np.int64)
    if name == "edges":
        return np.arange(64, dtype=np.int64) % 10
    if name == "one_long":  # wave_nb far above most lanes' block count
        c = np.full(64, 2, dtype=np.int64)
        c[int(rng.integers(0, 64))] = ONE_LONG
        return c
    if name == "mixed":
        return rng.integers(0, 45, 64)
    if name == "zeros_mixed":
        c = rng.integers(1, 31, 64)
        c[::2] = 0
        return c
    assert name == "one_nb"
    c = rng.integers(2, 4, 64)
    c[0], c[1] = 2, 3
    return c


def _null_masks(name, counts, rng):
    masks = [np.zeros(int(c), dtype=bool) for c in counts]
    if name == "lane0_first":
        masks[0][:1] = True
    elif name == "lane63_last":
        masks[63][-1:] = True
    elif name == "lane31_all":
        masks[31][:] = True
    elif name == "each_one":
        want = list(PREFETCHED)
        for m in masks:
            if m.size:
                # behind the two entries read up front wherever the list is that long, or a
                # lane with its null at 0 or 1 would decide the ballot for all 64
                p = int(rng.integers(2 if m.size > 2 else 0, m.size))
                if want and m.size > want[0]:
                    p = want.pop(0)
                m[p] = True
    elif name == "half":
        masks = [rng.random(m.size) < 0.5 for m in masks]
    elif name == "all_null":
        for m in masks:
            m[:] = True
    else:
        assert name == "none"
    return masks


def _entries(name, masks, rng):
    shared = rng.integers(0, N_DIGESTS, max(m.size for m in masks) if masks else 0)
    out = []
    for m in masks:
        v = shared[:m.size].copy() if name == "shared" else rng.integers(0, N_DIGESTS, m.size)
        if name == "edge":  # the first and the last row the digest descriptor admits
            live = np.flatnonzero(~m)
            if live.size:
                v[live[0]] = 0
                v[live[-1]] = N_DIGESTS - 1
        v[m] = K_NULL_INDEX
        out.append(v)
    return out


def build(seed=0):
    """(idx, first, n_digests, meta): meta[g] = (counts, nulls, indices) of group g."""
    meta = [(c, nl, ix) for c in COUNTS for nl in NULLS for ix in INDICES]
    sizes, entries = [], []
    for g, (c, nl, ix) in enumerate(meta):
        rng = np.random.default_rng([seed, 79, g])
        counts = _counts(c, rng)
        masks = _null_masks(nl, counts, rng)
        sizes.append(counts)
        entries.extend(_entries(ix, masks, rng))
    first = np.concatenate([[0], np.cumsum(np.concatenate(sizes))]).astype(np.uint32)
    idx = np.concatenate(entries).astype(np.uint32)
    assert first[-1] == idx.size and first[-1] > first[-2]
    return idx, first, N_DIGESTS, meta


def group_index(meta, counts, nulls, indices):
    return meta.index((counts, nulls, indices))


def with_partial_group(first, idx, group, r):
    """The stream's first `group` groups, then the first r lists of group `group`
    as a partial last wave: (idx, first) with first[-1] == idx.size."""
    n = 64 * group + r
    f = first[:n + 1].copy()
    return idx[:int(f[-1])].copy(), f


def repeat_rotated(idx, first, n_groups, step=29):
    """The stream repeated to n_groups groups, repetition j rotated by step * j
    lists (no multiple of 64, so its groups differ from every other
    repetition's): (idx, first, src) with src[k] = the stream's list behind list k."""
    first = np.asarray(first, dtype=np.int64)
    n0 = first.size - 1
    slot = np.arange(64 * n_groups)
    rep = slot // n0
    assert ((step * np.arange(1, int(rep[-1]) + 1)) % 64 != 0).all()
    src = (slot + step * rep) % n0
    counts = (first[1:] - first[:-1])[src]
    f = np.concatenate([[0], np.cumsum(counts)])
    pos = np.repeat(first[:-1][src], counts) + np.arange(int(f[-1])) - np.repeat(f[:-1], counts)
    return np.asarray(idx)[pos].astype(np.uint32), f.astype(np.uint32), src


def uniform(n, B):
    """Identity BatchSize lists over n digests: (idx, first)."""
    return sharding.batch_lists(n, B)


def _shape(c, valid):
    big = np.int64(1) << 40
    mx, mn = np.where(valid, c, 0).max(axis=1), np.where(valid, c, big).min(axis=1)
    nb = blocks_for_count(c)
    nb_mx, nb_mn = np.where(valid, nb, 0).max(axis=1), np.where(valid, nb, big).min(axis=1)
    uni = mx == mn
    shape = np.where(uni & (mx % 2 == 0), "uni_even",
                     np.where(uni, "uni_odd", np.where(nb_mx == nb_mn, "mixed_one_nb", "mixed_nb")))
    return shape, nb_mx


def classify(idx, first):
    """The wave-wide predicates per group of 64 lists (the last may be partial).

    Raw view (sha256_lists_kernel, which sees idx as it is): raw_nulls of
    RAW_NULLS by the number of lanes that hold a null, raw_shape of SHAPES over
    the raw counts, raw_wave_nb.  Compacted view (every plan form, after the
    host dropped the nulls): shape of SHAPES, has_empty, wave_nb and chunks =
    ceil(wave_nb / kFusedChunkBlocks), the group's readiness counters."""
    idx = np.asarray(idx, dtype=np.uint32)
    first = np.asarray(first, dtype=np.int64)
    n_lists = first.size - 1
    n_groups = (n_lists + 63) // 64
    seen = np.concatenate([[0], np.cumsum(idx == K_NULL_INDEX)])
    raw = np.zeros(64 * n_groups, dtype=np.int64)
    nul = np.zeros(64 * n_groups, dtype=np.int64)
    raw[:n_lists] = first[1:] - first[:-1]
    nul[:n_lists] = seen[first[1:]] - seen[first[:-1]]
    valid = (np.arange(64 * n_groups) < n_lists).reshape(n_groups, 64)
    raw, nul = raw.reshape(n_groups, 64), nul.reshape(n_groups, 64)
    lanes = (valid & (nul > 0)).sum(axis=1)
    raw_shape, raw_nb = _shape(raw, valid)
    shape, wave_nb = _shape(raw - nul, valid)
    return {"raw_nulls": np.where(lanes == 0, "none", np.where(lanes == 1, "one_lane", "several_lanes")),
            "raw_shape": raw_shape, "raw_wave_nb": raw_nb,
            "shape": shape, "has_empty": (valid & (raw == nul)).any(axis=1), "wave_nb": wave_nb,
            "chunks": (wave_nb + K_FUSED_CHUNK_BLOCKS - 1) // K_FUSED_CHUNK_BLOCKS}


def raw_census(cls):
    """Group count per cell of RAW_CELLS."""
    got = list(zip(cls["raw_nulls"].tolist(), cls["raw_shape"].tolist()))
    return {c: got.count(c) for c in RAW_CELLS}


def compacted_census(cls):
    """Per compacted shape of SHAPES: (groups, groups that hold an empty list)."""
    return {s: (int((cls["shape"] == s).sum()), int(((cls["shape"] == s) & cls["has_empty"]).sum())) for s in SHAPES}
