"""The range-check contracts that include/mirsha.h states for the two calls
whose offsets, lengths and indices live in device memory, where the library
cannot validate them: mirsha_digest_lists_device (an index in [n_digests,
MIRSHA_NULL_INDEX) reads 32 zero bytes, whatever its value) and
mirsha_hash_batch_device (reads at or past arena_len rounded up to 4 return 0;
one descriptor up to MIRSHA_MAX_DEVICE_ARENA_BYTES, the 64-bit loader beyond).
Both hashers, every kernel a launch can take, against hashlib over the models
of tests/contract_cases.py, bit-exact.  tests/test_contract_cases_cpu.py shows
on the CPU that these cases tell a wrong loader from a right one and that none
of them can touch memory outside its allocation.

Every buffer is a torch tensor of exactly the size the call is told (the table
and the arenas carry the slack the cases are built for), outputs are pre-filled
with 0xEE and end in canary rows."""
import numpy as np
import pytest

import contract_cases as cc
from mirbft_amd import Engine, bucket_order, sha512_pair_max_groups
from mirbft_amd.engine import (VARIANT_CU, VARIANT_DIRECT, VARIANT_LDS, VARIANT_LDS_ONLY, VARIANT_LOWOCC,
                               VARIANT_PAIR)

pytestmark = pytest.mark.gpu
CANARY = 0xEE
KMAX = cc.K_MAX_BUFFER_ARENA
SHA256_VARIANTS = [VARIANT_LDS, VARIANT_DIRECT, VARIANT_LOWOCC, VARIANT_LDS_ONLY, VARIANT_PAIR, VARIANT_CU]
SHA256_IDS = ["lds", "direct", "lowocc", "lds_only", "pair", "cu"]
# SHA-512/256: 5 = the one-lane kernel at any size, 0 = automatic, the pair kernel for these small launches
SHA512_VARIANTS = [VARIANT_LDS_ONLY, VARIANT_LDS]
SHA512_IDS = ["one_lane", "pair"]


def _torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def dev(a: np.ndarray):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def own(engine):
    """An engine of this module's own (after the session's, so torch's runtime
    came up first): a failing test cannot leave the shared one on SHA-512/256."""
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture()
def e512(own):
    own.set_hasher("sha512_256")
    own.set_order_mode("host")
    own.set_variant(VARIANT_LDS)
    yield own
    own.set_variant(VARIANT_LDS)
    own.set_hasher("sha256")


@pytest.fixture()
def e256(engine):
    engine.set_variant(VARIANT_LDS)
    yield engine
    engine.set_variant(VARIANT_LDS)


class Route:
    """with Route(eng, k): the block queues exactly k SHA-512/256 pair launches."""

    def __init__(self, eng, launches):
        self.eng, self.launches = eng, launches

    def __enter__(self):
        self.before = self.eng.sha512_pair_launches

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            got = self.eng.sha512_pair_launches - self.before
            assert got == self.launches, f"{got} pair launches, {self.launches} expected"


def wrong(cases, got, want):
    """The names of the cases whose digest differs."""
    return [cases[k][0] for k in np.flatnonzero((got != want).any(axis=1)).tolist()]


# ---- a. out-of-range indices ---------------------------------------------------
@pytest.fixture(scope="module")
def table():
    tab = cc.table()
    return tab, dev(tab)  # the device tensor holds N_ROWS rows, the calls pass N_DIGESTS


def run_lists(eng, d_table, n_digests, lists) -> np.ndarray:
    torch = _torch()
    idx, first = cc.flatten(lists)
    d_first = dev(first.view(np.int32))
    d_idx = dev((idx if idx.size else np.zeros(1, dtype=np.uint32)).view(np.int32))
    d_out = torch.full((len(lists) + 4, 32), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # torch's stream vs the engine's own (non-blocking) stream
    eng.digest_lists_device(d_table.data_ptr(), n_digests, d_idx.data_ptr(), d_first.data_ptr(), len(lists),
                            int(idx.size), d_out.data_ptr())
    eng.sync()
    out = d_out.cpu().numpy()
    assert (out[len(lists):] == CANARY).all()
    return out[:len(lists)]


def check_lists(eng, hasher, table, lists, n_digests=cc.N_DIGESTS):
    tab, d_table = table
    got = run_lists(eng, d_table, n_digests, lists)
    bad = wrong(lists, got, cc.want_lists(hasher, tab, n_digests, lists))
    assert not bad, f"{len(bad)} of {len(lists)} lists differ: {bad[:40]}"


@pytest.mark.parametrize("kind", ["no_null", "nulls"])
def test_sha256_out_of_range_indices_read_zeros(e256, table, kind):
    """no_null: the optimistic pass alone; nulls: every wave compacts into
    scratch and hashes again."""
    check_lists(e256, "sha256", table, cc.list_launch(kind))


def test_sha256_out_of_range_index_in_a_launch_of_one_list(e256, table):
    for lists in cc.single_list_launches():
        check_lists(e256, "sha256", table, lists)


@pytest.mark.parametrize("kind", ["no_null", "nulls"])
def test_sha512_pair_out_of_range_indices_read_zeros(e512, table, kind):
    lists = cc.list_launch(kind)
    assert (len(lists) + 63) // 64 <= sha512_pair_max_groups()
    with Route(e512, 1):
        check_lists(e512, "sha512_256", table, lists)


def test_sha512_pair_out_of_range_index_in_a_launch_of_one_list(e512, table):
    for lists in cc.single_list_launches():
        with Route(e512, 1 if sha512_pair_max_groups() else 0):
            check_lists(e512, "sha512_256", table, lists)


def test_sha512_one_lane_out_of_range_indices_read_zeros(e512, table):
    """The same lists tiled past the pair threshold: sha512_lists_kernel."""
    lists = cc.tiled(cc.list_launch("nulls"), 64 * sha512_pair_max_groups() + 1)
    with Route(e512, 0):
        check_lists(e512, "sha512_256", table, lists)


def test_sha256_empty_table(e256, table):
    check_lists(e256, "sha256", table, cc.empty_table_launch(), n_digests=0)


def test_sha512_empty_table(e512, table):
    check_lists(e512, "sha512_256", table, cc.empty_table_launch(), n_digests=0)


# ---- b. reads past arena_len ---------------------------------------------------------
def run_msgs(eng, d_arena, arena_len, msgs, order=False) -> np.ndarray:
    torch = _torch()
    off, ln = cc.arrays(msgs)
    n = len(msgs)
    d_off, d_len = dev(off.view(np.int64)), dev(ln.view(np.int32))
    d_order = dev(bucket_order(ln)[0].view(np.int32)) if order else None
    d_out = torch.full((n + 4, 32), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # torch's stream vs the engine's own (non-blocking) stream
    eng.hash_batch_device(d_arena.data_ptr(), int(arena_len), d_off.data_ptr(), d_len.data_ptr(),
                          None if d_order is None else d_order.data_ptr(), n, d_out.data_ptr())
    eng.sync()
    out = d_out.cpu().numpy()
    assert (out[n:] == CANARY).all()
    return out[:n]


def check_msgs(eng, hasher, read, d_arena, arena_len, msgs, order=False):
    got = run_msgs(eng, d_arena, arena_len, msgs, order)
    bad = wrong(msgs, got, cc.want_arena(hasher, read, cc.rounded(arena_len), msgs))
    assert not bad, f"arena_len {arena_len}: {len(bad)} of {len(msgs)} messages differ: {bad[:40]}"


@pytest.fixture(scope="module")
def small_arenas():
    """(host bytes, device tensor) of the 4096-byte allocation and of the
    uniform tile's; none of their bytes is zero."""
    a = cc.nonzero_bytes(np.random.default_rng([7, 6]), cc.ARENA_ALLOC)
    t = cc.nonzero_bytes(np.random.default_rng([7, 7]), cc.TILE_ALLOC)
    return (a, dev(a)), (t, dev(t))


def check_small_arenas(eng, hasher, small_arenas, r):
    (a, d_a), (t, d_t) = small_arenas
    A = cc.ARENA_LENS[r]
    check_msgs(eng, hasher, cc.reader(a), d_a, A, cc.overhang_messages(A))
    # one uniform 4-byte aligned tile whose last messages overhang: SHA-256's uni, aligned and
    # tail-form branches with `far` false
    check_msgs(eng, hasher, cc.reader(t), d_t, cc.TILE_ARENA_LENS[r], cc.tile_messages())


@pytest.mark.parametrize("r", [0, 1, 2, 3])
@pytest.mark.parametrize("variant", SHA256_VARIANTS, ids=SHA256_IDS)
def test_sha256_reads_at_or_past_the_rounded_arena_len_are_zero(e256, small_arenas, variant, r):
    e256.set_variant(variant)
    check_small_arenas(e256, "sha256", small_arenas, r)


@pytest.mark.parametrize("r", [0, 1, 2, 3])
@pytest.mark.parametrize("variant", SHA512_VARIANTS, ids=SHA512_IDS)
def test_sha512_reads_at_or_past_the_rounded_arena_len_are_zero(e512, small_arenas, variant, r):
    e512.set_variant(variant)
    with Route(e512, 2 if variant == VARIANT_LDS else 0):
        check_small_arenas(e512, "sha512_256", small_arenas, r)


# ---- c. the top of the descriptor and the loader switch ----------------------------------
@pytest.fixture(scope="module")
def top():
    """One allocation of kMaxBufferArena + 8192 bytes, never written as a whole:
    three windows are filled from host arrays, the reference reads those."""
    torch = _torch()
    w = cc.Windows()
    d = torch.empty(cc.TOP_ALLOC, dtype=torch.uint8, device="cuda")
    for base, part in w.parts:
        d[base:base + part.size].copy_(torch.from_numpy(part))
    torch.cuda.synchronize()
    yield w, d
    del d
    torch.cuda.empty_cache()


@pytest.mark.parametrize("order", [False, True], ids=["identity", "bucket_order"])
@pytest.mark.parametrize("variant", SHA256_VARIANTS, ids=SHA256_IDS)
def test_sha256_arena_of_exactly_one_descriptor(e256, top, variant, order):
    w, d = top
    e256.set_variant(variant)
    check_msgs(e256, "sha256", w.read, d, KMAX, cc.top_messages(KMAX), order)


@pytest.mark.parametrize("order", [False, True], ids=["identity", "bucket_order"])
@pytest.mark.parametrize("extra", [1, 4])
def test_sha256_one_byte_more_takes_the_64_bit_loader(e256, top, extra, order):
    """The last message ends exactly at the new arena_len."""
    w, d = top
    check_msgs(e256, "sha256", w.read, d, KMAX + extra, cc.top_messages(KMAX + extra), order)


@pytest.mark.parametrize("variant", SHA256_VARIANTS, ids=SHA256_IDS)
def test_sha256_overhang_at_the_top_of_the_descriptor(e256, top, variant):
    """Group b's messages around an arena_len of every residue just below
    kMaxBufferArena; off + len stays below 2^32, as the header requires."""
    w, d = top
    e256.set_variant(variant)
    for A in range(KMAX - 3, KMAX + 1):
        check_msgs(e256, "sha256", w.read, d, A, cc.overhang_messages(A, end_below=1 << 32))


@pytest.mark.parametrize("order", [False, True], ids=["identity", "bucket_order"])
@pytest.mark.parametrize("variant", SHA512_VARIANTS, ids=SHA512_IDS)
def test_sha512_arena_of_exactly_one_descriptor(e512, top, variant, order):
    w, d = top
    e512.set_variant(variant)
    with Route(e512, 1 if variant == VARIANT_LDS else 0):
        check_msgs(e512, "sha512_256", w.read, d, KMAX, cc.top_messages(KMAX), order)


@pytest.mark.parametrize("variant", SHA512_VARIANTS, ids=SHA512_IDS)
def test_sha512_overhang_at_the_top_of_the_descriptor(e512, top, variant):
    w, d = top
    e512.set_variant(variant)
    for A in range(KMAX - 3, KMAX + 1):
        check_msgs(e512, "sha512_256", w.read, d, A, cc.overhang_messages(A, end_below=1 << 32))
