"""Deterministic cases at and past the edges of the ranges that the
device-pointer calls check on the device (include/mirsha.h,
mirsha_digest_lists_device and mirsha_hash_batch_device), and the reference for
them: hashlib over the two models the header states.  Test infrastructure.

  lists   row i of the table when i < n_digests, 32 zero bytes otherwise;
          MIRSHA_NULL_INDEX entries are skipped
  arenas  the allocation's bytes below R = arena_len rounded up to a multiple
          of 4, zeros from R onward

Every case is safe under a loader with no range check at all: a message's
off + len + 132 lies inside its allocation, and every index that such a loader
would turn into a row lies inside the table's allocation, so a wrong kernel
gives a wrong digest, never a fault.

The wrong models (tests/test_contract_cases_cpu.py) restate the ways a loader
can miss the contract; the cases they get wrong are predicted here from
interval arithmetic alone (wraps(), reads_at_or_past(), reads_the_partial_word()).
"""
import hashlib

import numpy as np

# Restated from include/mirsha.h and mirbft_amd/csrc/mirsha_kernels.h
# (tests/test_contract_cases_cpu.py compares them with the headers' text).
NULL = 0xFFFFFFFF
K_MAX_LIST_DIGESTS = (1 << 27) - 1
K_MAX_BUFFER_ARENA = 0xFFFFFF00

# The widest access of any loader past a message's first byte: SHA-512's 33
# dwords of a block (sha512_lanes.h); SHA-256's chunks take 20 bytes.
SLACK = 132


def H(hasher, b) -> bytes:
    return hashlib.new(hasher, bytes(b)).digest()


def rows(digests) -> np.ndarray:
    return np.frombuffer(b"".join(digests), dtype=np.uint8).reshape(-1, 32)


def nonzero_bytes(rng, size) -> np.ndarray:
    """Every byte 1..255: a byte that reads as zero shows, whatever it was."""
    return rng.integers(1, 256, size=size, dtype=np.uint8)


# ---- lists -------------------------------------------------------------------
N_DIGESTS = 77    # the rows the call is told about
N_ROWS = 85       # the rows the table's allocation holds
CONTROLS = (0, 76)
SLACK_ROWS = (77, 78, 84)  # out of range, inside the allocation
OUT_OF_RANGE = SLACK_ROWS + ((1 << 27) - 1, 1 << 27, (1 << 27) + 5, (1 << 27) + 76, (1 << 28) + 1, 1 << 31,
                             (1 << 31) + 3, 0xFFFFFFFE)
# name -> the list around v: the two-rows-a-block edge of SHA-256 and the
# four-rows-a-block edge of SHA-512, v first, last and alone, v beside nulls
SHAPES = {
    "v": lambda v: [v],
    "5_v": lambda v: [5, v],
    "v_5": lambda v: [v, 5],
    "1_2_3_v": lambda v: [1, 2, 3, v],
    "1_2_3_4_v": lambda v: [1, 2, 3, 4, v],
    "null_v_5": lambda v: [NULL, v, 5],
    "v_null": lambda v: [v, NULL],
    "v_x5": lambda v: [v] * 5,
}
NULL_SHAPES = ("null_v_5", "v_null")


def table():
    """(N_ROWS, 32) bytes, none zero; the call passes the first N_DIGESTS rows."""
    return nonzero_bytes(np.random.default_rng([7, 1]), (N_ROWS, 32))


def _fillers(rng):
    """All-in-range lists of 0..9 entries that sit beside the cases in a wave."""
    return [(("fill", c), rng.integers(0, N_DIGESTS, size=c).tolist()) for c in range(10)]


def list_launch(kind):
    """[(name, ids)] of one launch; name = (v, shape) or ("fill", count).

    no_null  every NULL-free shape of every value but NULL: sha256_lists_kernel
             runs its optimistic pass alone
    nulls    every shape of every value, NULL as a value included: each
             64-list wave holds NULL entries, so it compacts and hashes again"""
    rng = np.random.default_rng([7, 2, ("no_null", "nulls").index(kind)])
    fill = _fillers(rng)
    values = CONTROLS + OUT_OF_RANGE + ((NULL,) if kind == "nulls" else ())
    out = []
    for j, v in enumerate(values):
        for name, make in SHAPES.items():
            if kind == "nulls" or name not in NULL_SHAPES:
                out.append(((v, name), make(v)))
        if j < len(fill):
            out.append(fill[j])
    return out


def single_list_launches():
    """One launch of one list per out-of-range value: n_lists = 1."""
    return [[((v, "5_v"), SHAPES["5_v"](v))] for v in OUT_OF_RANGE]


def empty_table_launch():
    """n_digests = 0 with a valid table pointer: every row reads zeros."""
    return [((0, "v"), [0]), ((5, "v_null"), [5, NULL]), (("fill", 0), [])]


def tiled(lists, n):
    """`lists` repeated to n lists."""
    return [lists[k % len(lists)] for k in range(n)]


def flatten(lists):
    """(idx, first) of [(name, ids)]; idx never empty (a descriptor needs a base)."""
    idx = np.asarray([i for _, ids in lists for i in ids], dtype=np.uint32)
    first = np.concatenate([[0], np.cumsum([len(ids) for _, ids in lists])]).astype(np.uint32)
    return idx, first


def row_contract(tab, n_digests, i):
    return tab[i].tobytes() if i < n_digests else bytes(32)


def row_wrapping(tab, n_digests, i):
    """Wrong model 1: the row's byte offset taken modulo 2^32, then checked
    against 32 n_digests -- a 32-bit multiply ahead of the range check."""
    o = (32 * i) & 0xFFFFFFFF
    return tab[o // 32].tobytes() if o + 32 <= 32 * n_digests else bytes(32)


def list_message(tab, n_digests, ids, row=row_contract) -> bytes:
    return b"".join(row(tab, n_digests, i) for i in ids if i != NULL)


def want_lists(hasher, tab, n_digests, lists, row=row_contract) -> np.ndarray:
    memo = {}
    for _, ids in lists:
        key = tuple(ids)
        if key not in memo:
            memo[key] = H(hasher, list_message(tab, n_digests, ids, row))
    return rows([memo[tuple(ids)] for _, ids in lists])


def wraps(ids, n_digests=N_DIGESTS):
    """The list holds an index whose 32-bit row offset lands on a row in range."""
    return any(i != NULL and i >= 1 << 27 and i % (1 << 27) < n_digests for i in ids)


# ---- arenas --------------------------------------------------------------------
ARENA_ALLOC = 4096
ARENA_LENS = (1000, 1001, 1002, 1003)
# k = 7 is added to the issue's {0, 1, 5, 64, 130}: with it k takes every
# residue mod 4, so every overhang meets every byte alignment under every
# arena_len mod 4.
INSIDE = (0, 1, 5, 7, 64, 130)
OVERHANG = (1, 2, 3, 4, 5, 17, 63, 64, 65, 127, 128, 129, 200)
PAST = (0, 1, 7, 300)
PAST_LENS = (0, 1, 55, 56, 111, 112, 200)
# (bytes back from arena_len, length): wholly inside; (130, 130) and (1, 1) end exactly at arena_len
CONTROL_MSGS = ((900, 0), (899, 1), (850, 55), (777, 56), (700, 63), (650, 64), (601, 65), (500, 111), (480, 112),
                (350, 119), (343, 120), (340, 127), (338, 128), (333, 129), (300, 200), (290, 272), (130, 130), (1, 1))


def rounded(arena_len):
    return (arena_len + 3) & ~3


def overhang_messages(arena_len, end_below=None):
    """[(cls, off, len)] around arena_len, shuffled so that a wave mixes the
    classes.  cls = ("partial", k, h), ("past", d, L) or ("control", back, L).
    end_below: keep only messages with off + len < end_below."""
    msgs = [(("partial", k, h), arena_len - k, k + h) for k in INSIDE for h in OVERHANG]
    msgs += [(("past", d, L), arena_len + d, L) for d in PAST for L in PAST_LENS]
    msgs += [(("control", back, L), arena_len - back, L) for back, L in CONTROL_MSGS]
    if end_below is not None:
        msgs = [m for m in msgs if m[1] + m[2] < end_below]
    p = np.random.default_rng([7, 3, arena_len & 3]).permutation(len(msgs))
    return [msgs[i] for i in p]


TILE_N, TILE_LEN = 64, 272
TILE_ALLOC = TILE_N * TILE_LEN + 256
TILE_ARENA_LENS = (17000, 17001, 17002, 17003)


def tile_messages():
    """One uniform tile: 64 x 272 bytes back to back from 0, 4-byte aligned.
    Under TILE_ARENA_LENS message 62 overhangs and message 63 lies wholly past."""
    return [(("tile", i), TILE_LEN * i, TILE_LEN) for i in range(TILE_N)]


def arena_message(read, zero_from, off, ln) -> bytes:
    """The message's bytes: read(a, b) below zero_from, zeros from there on."""
    real = max(0, min(off + ln, zero_from) - off)
    return (read(off, off + real) if real else b"") + bytes(ln - real)


def reader(alloc: np.ndarray):
    return lambda a, b: alloc[a:b].tobytes()


def want_arena(hasher, read, zero_from, msgs) -> np.ndarray:
    return rows([H(hasher, arena_message(read, zero_from, off, ln)) for _, off, ln in msgs])


def reads_at_or_past(zero_from, off, ln):
    """The message holds a byte at or past zero_from."""
    return off + ln > zero_from and ln > 0


def reads_the_partial_word(arena_len, off, ln):
    """The message holds a byte of [arena_len, R): real under the contract,
    zero under a check against arena_len itself."""
    return max(off, arena_len) < min(off + ln, rounded(arena_len))


def arrays(msgs):
    return (np.asarray([o for _, o, _ in msgs], dtype=np.uint64), np.asarray([n for _, _, n in msgs], dtype=np.uint32))


# ---- the top of the descriptor ---------------------------------------------------
TOP_ALLOC = K_MAX_BUFFER_ARENA + 8192
MID = 1 << 31
WINDOWS = ((0, 64 << 10), (MID - 4096, MID + 4096), (K_MAX_BUFFER_ARENA - (64 << 10), TOP_ALLOC))


class Windows:
    """The filled windows of the large allocation as host arrays; read() serves
    only bytes inside one window (the rest of the allocation is never written,
    so no case may depend on it)."""

    def __init__(self):
        rng = np.random.default_rng([7, 4])
        self.parts = [(a, nonzero_bytes(rng, b - a)) for a, b in WINDOWS]

    def read(self, a, b):
        for base, w in self.parts:
            if base <= a and b <= base + w.size:
                return w[a - base:b - base].tobytes()
        raise AssertionError(f"[{a}, {b}) is in no window")


def _packed(rng, lengths, pos):
    """Messages back to back from pos, message j at byte alignment (pos + j) % 4."""
    out, a0 = [], pos % 4
    for j, L in enumerate(lengths):
        pos += ((a0 + j) % 4 - pos) % 4
        out.append((pos, int(L)))
        pos += int(L)
    return out


def top_messages(arena_len=K_MAX_BUFFER_ARENA):
    """[(cls, off, len)]: about 130 messages of 0..700 bytes at the start of the
    arena (behind a lead of 3 bytes), straddling 2^31 (one of 5000 bytes among
    them) and in the top window, the last one ending exactly at arena_len."""
    rng = np.random.default_rng([7, 5])
    msgs = [(("start", j), o, L) for j, (o, L) in enumerate(_packed(rng, rng.integers(0, 701, size=44), 3))]
    for j in range(40):  # message j starts 1 + 17 j bytes below 2^31: every alignment, ends past 2^31
        back = 1 + 17 * j
        msgs.append((("mid", j), MID - back, back + int(rng.integers(1, 701 - back + 1))))
    msgs.append((("mid", "long"), MID - 2501, 5000))
    lengths = rng.integers(0, 701, size=45)
    lengths[-1] = 333
    rel = _packed(rng, lengths, 0)
    base = arena_len - (rel[-1][0] + rel[-1][1])
    msgs += [(("top", j), base + o, L) for j, (o, L) in enumerate(rel)]
    return msgs
