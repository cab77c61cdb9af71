"""The producer/consumer pair route of SHA-512/256 on the device
(mirsha_sha512_pair.hip): small request, list and sequential-plan launches
split every compression over two waves.  Against hashlib, bit-exact, and every
case also asserts the route by the change of Engine.sha512_pair_launches: +1 for
each launch that must take a pair kernel, +0 where the one-lane kernels must
run.  The shapes are the smallest at which the pair kernels can still go wrong:
every padding case at every byte alignment inside one launch (lanes of
different block counts in a wave), partial groups, a long lane beside finished
ones, the arena's end (the single-dword loader inside the producer), lists
around the four-rows-a-block boundary with nulls (the walked trip count), and
both sides of the threshold, which is read from the library."""
import hashlib

import numpy as np
import pytest

from mirbft_amd import Engine, _lib, sha512_pair_max_groups, sharding
from test_gpu_sha512 import H, _torch, dev, hash_device, packed, rows, want_batch

pytestmark = pytest.mark.gpu
NULL = _lib.MIRSHA_NULL_INDEX
CANARY = 0xEE


@pytest.fixture(scope="module")
def own(engine):
    """An engine of this module's own (after the session's, so torch's runtime
    came up first): a failing test cannot leave the shared one on SHA-512/256."""
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture()
def eng(own):
    own.set_hasher("sha512_256")
    own.set_order_mode("host")
    own.set_variant(0)
    yield own
    own.set_variant(0)
    own.set_hasher("sha256")


class Route:
    """with Route(eng, k): the block queues exactly k pair launches."""

    def __init__(self, eng, launches):
        self.eng, self.launches = eng, launches

    def __enter__(self):
        self.before = self.eng.sha512_pair_launches

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            got = self.eng.sha512_pair_launches - self.before
            assert got == self.launches, f"{got} pair launches, {self.launches} expected"


def groups(n: int) -> int:
    return (n + 63) // 64


# messages -------------------------------------------------------------------
@pytest.fixture(scope="module")
def every_padding_case():
    """Every length 0..300 at each of the four byte alignments: 1,204 messages,
    19 groups; the reference is computed once."""
    rng = np.random.default_rng(1)
    lengths = [L for L in range(301) for _ in range(4)]
    arena, off, ln = packed(lengths, rng, align=lambda k: k % 4)
    assert sorted(set((off % 4).tolist())) == [0, 1, 2, 3] and off.size == 1204
    return arena, off, ln, want_batch(arena, off, ln), rng.permutation(off.size).astype(np.uint32)


def test_every_padding_case_at_every_alignment_in_one_launch(eng, every_padding_case):
    arena, off, ln, want, shuffled = every_padding_case
    assert groups(off.size) == 19 <= sha512_pair_max_groups()
    with Route(eng, 1):
        got = hash_device(eng, arena, off, ln)
    assert np.array_equal(got, want)
    with Route(eng, 1):  # a wave now holds lanes of different block counts
        got = hash_device(eng, arena, off, ln, shuffled)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_partial_last_group(eng, n):
    rng = np.random.default_rng(100 + n)
    arena, off, ln = packed(rng.integers(0, 701, size=n).tolist(), rng, lead=3)
    with Route(eng, 1):
        got = hash_device(eng, arena, off, ln)
    assert np.array_equal(got, want_batch(arena, off, ln))


def test_a_long_live_lane_beside_finished_ones(eng):
    rng = np.random.default_rng(4)
    lengths = rng.integers(0, 41, size=64).tolist()
    lengths[17] = 61_600  # 482 blocks
    arena, off, ln = packed(lengths, rng, lead=1)
    with Route(eng, 1):
        got = hash_device(eng, arena, off, ln)
    assert np.array_equal(got, want_batch(arena, off, ln))


@pytest.mark.parametrize("align", [1, 2, 3])
def test_last_message_ends_at_an_arena_length_that_is_no_multiple_of_4(eng, align):
    """The arena's last block takes the producer's single-dword loads."""
    rng = np.random.default_rng(300 + align)
    for tail in (1, 2, 3, 17, 130, 257):
        start = 8 + align
        while (start + tail) % 4 == 0:
            start += 1
        arena = rng.integers(1, 256, size=start + tail, dtype=np.uint8)  # no zero byte: zeros would show
        off, ln = np.array([0, start], dtype=np.uint64), np.array([5, tail], dtype=np.uint32)
        assert arena.size % 4 != 0 and int(off[1]) + int(ln[1]) == arena.size
        with Route(eng, 1):
            got = hash_device(eng, arena, off, ln)
        assert np.array_equal(got, want_batch(arena, off, ln)), (align, tail)


@pytest.fixture(scope="module")
def threshold_messages():
    """One message more than the largest launch that takes the pair, 33 bytes each."""
    n = 64 * sha512_pair_max_groups() + 1
    arena = np.random.default_rng(5).integers(0, 256, size=33 * n, dtype=np.uint8)
    off = np.arange(n, dtype=np.uint64) * 33
    ln = np.full(n, 33, dtype=np.uint32)
    return arena, off, ln, want_batch(arena, off, ln)


def test_both_sides_of_the_threshold(eng, threshold_messages):
    arena, off, ln, want = threshold_messages
    n = off.size
    if n > 1:
        with Route(eng, 1):
            got = hash_device(eng, arena[: 33 * (n - 1)], off[: n - 1], ln[: n - 1])
        assert np.array_equal(got, want[: n - 1])
    with Route(eng, 0):
        got = hash_device(eng, arena, off, ln)
    assert np.array_equal(got, want)


def test_variants_force_either_kernel(eng, every_padding_case):
    arena, off, ln, want, _ = every_padding_case
    try:
        eng.set_variant(5)
        with Route(eng, 0):
            got = hash_device(eng, arena, off, ln)
        assert np.array_equal(got, want)
        n = 40_000
        assert groups(n) > sha512_pair_max_groups()
        big = np.random.default_rng(6).integers(0, 256, size=33 * n, dtype=np.uint8)
        boff, bln = np.arange(n, dtype=np.uint64) * 33, np.full(n, 33, dtype=np.uint32)
        eng.set_variant(6)
        with Route(eng, 1):
            got = hash_device(eng, big, boff, bln)
        assert np.array_equal(got, want_batch(big, boff, bln))
    finally:
        eng.set_variant(0)
    with Route(eng, 1):
        got = hash_device(eng, arena, off, ln)
    assert np.array_equal(got, want)


# lists ----------------------------------------------------------------------
def lists_device(eng, table, lists):
    torch = _torch()
    idx = np.asarray([i for ids in lists for i in ids], dtype=np.uint32)
    first = np.concatenate([[0], np.cumsum([len(ids) for ids in lists])]).astype(np.uint32)
    d_table, d_first = dev(table), dev(first.view(np.int32))
    d_idx = dev((idx if idx.size else np.zeros(1, dtype=np.uint32)).view(np.int32))
    d_out = torch.full((len(lists) + 4, 32), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.digest_lists_device(d_table.data_ptr(), table.shape[0], d_idx.data_ptr(), d_first.data_ptr(), len(lists),
                            int(idx.size), d_out.data_ptr())
    eng.sync()
    out = d_out.cpu().numpy()
    assert (out[len(lists):] == CANARY).all()
    return out[: len(lists)]


def want_lists(table, lists):
    return rows([H(b"".join(table[i].tobytes() for i in ids if i != NULL)) for ids in lists])


@pytest.fixture(scope="module")
def table():
    return np.random.default_rng(7).integers(0, 256, size=(600, 32), dtype=np.uint8)


def test_list_sizes_with_nulls_in_one_launch(eng, table):
    rng = np.random.default_rng(8)
    lists = []
    for c in range(14):
        ids = rng.integers(0, table.shape[0], size=c).tolist()
        lists += [ids, [NULL] + ids, ids[: c // 2] + [NULL, NULL] + ids[c // 2:], ids + [NULL], [NULL] * c]
    with Route(eng, 1):
        got = lists_device(eng, table, lists)
    assert np.array_equal(got, want_lists(table, lists))
    assert got[0].tobytes() == got[4 * 5 + 4].tobytes() == H(b"")  # empty, and four nulls


def test_nine_lists_of_up_to_500(eng, table):
    rng = np.random.default_rng(9)
    lists = [rng.integers(0, table.shape[0], size=c).tolist() for c in (1, 63, 125, 188, 250, 313, 375, 438, 500)]
    with Route(eng, 1):
        got = lists_device(eng, table, lists)
    assert np.array_equal(got, want_lists(table, lists))


@pytest.mark.parametrize("n_lists", [1, 64, 65])
def test_list_group_edges(eng, table, n_lists):
    rng = np.random.default_rng(500 + n_lists)
    lists = [rng.integers(0, table.shape[0], size=int(c)).tolist() for c in rng.integers(0, 12, size=n_lists)]
    lists[0] = [5, NULL, 5, 599, 0]
    with Route(eng, 1):
        got = lists_device(eng, table, lists)
    assert np.array_equal(got, want_lists(table, lists))


def test_repeated_and_descending_indices(eng, table):
    lists = [[9, 9, 9, 9, 9], [8, 7, 6, 5, 4, 3, 2, 1, 0]]
    with Route(eng, 1):
        got = lists_device(eng, table, lists)
    assert np.array_equal(got, want_lists(table, lists))


def test_many_short_lists_take_the_one_lane_kernel(eng, table):
    n_lists = 64 * sha512_pair_max_groups() + 1
    ids = np.random.default_rng(10).integers(0, table.shape[0], size=(n_lists, 2))
    lists = ids.tolist()
    with Route(eng, 0):
        got = lists_device(eng, table, lists)
    assert np.array_equal(got, want_lists(table, lists))


# plans ----------------------------------------------------------------------
def run_plan(eng, arena, off, ln, idx, first, launches):
    """One sequential SHA-512/256 plan run; returns (request rows, list rows)."""
    torch = _torch()
    n, n_lists = int(off.size), int(first.size) - 1
    d_arena, d_off, d_len = dev(arena), dev(off.view(np.int64)), dev(ln.view(np.int32))
    d_req = torch.full((n + 4, 32), CANARY, dtype=torch.uint8, device="cuda")
    d_bat = torch.full((n_lists + 4, 32), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    plan = eng.pipeline(n, idx, first, ln, mode="sequential", hasher="sha512_256")
    try:
        with Route(eng, launches):
            eng.hash_requests_then_batches_device(plan, d_arena.data_ptr(), int(arena.size), d_off.data_ptr(),
                                                  d_len.data_ptr(), d_req.data_ptr(), d_bat.data_ptr())
            eng.sync()
    finally:
        plan.close()
    req, bat = d_req.cpu().numpy(), d_bat.cpu().numpy()
    assert (req[n:] == CANARY).all() and (bat[n_lists:] == CANARY).all()
    return req[:n], bat[:n_lists]


def test_sequential_plan_identity_lists_with_a_partial_last_batch(eng):
    rng = np.random.default_rng(11)
    n = 610  # 31 batches of 20, the last of 10
    arena, off, ln = packed(rng.integers(0, 300, size=n).tolist(), rng)
    idx, first = sharding.batch_lists(n, 20)
    assert first.size - 1 == 31 and int(first[-1] - first[-2]) == 10
    req, bat = run_plan(eng, arena, off, ln, idx, first, launches=2)  # the request launch and the list launch
    want_req = want_batch(arena, off, ln)
    assert np.array_equal(req, want_req)
    assert np.array_equal(bat, want_lists(want_req, [idx[first[b]: first[b + 1]].tolist() for b in range(31)]))


def test_sequential_plan_loaded_indices_lists_of_500(eng):
    rng = np.random.default_rng(12)
    n = 700
    arena, off, ln = packed(rng.integers(0, 200, size=n).tolist(), rng)
    lists = [rng.integers(0, n, size=500).tolist(), [NULL] + rng.integers(0, n, size=499).tolist(),
             rng.integers(0, n, size=3).tolist(), []]
    idx = np.asarray([i for ids in lists for i in ids], dtype=np.uint32)
    first = np.concatenate([[0], np.cumsum([len(ids) for ids in lists])]).astype(np.uint32)
    req, bat = run_plan(eng, arena, off, ln, idx, first, launches=2)
    want_req = want_batch(arena, off, ln)
    assert np.array_equal(req, want_req)
    assert np.array_equal(bat, want_lists(want_req, lists))


def test_sequential_plan_above_the_threshold_takes_the_one_lane_kernels(eng):
    n = 64 * sha512_pair_max_groups() + 1  # as many lists of one entry
    arena = np.random.default_rng(13).integers(0, 256, size=8 * n, dtype=np.uint8)
    off, ln = np.arange(n, dtype=np.uint64) * 8, np.full(n, 8, dtype=np.uint32)
    idx, first = sharding.batch_lists(n, 1)
    req, bat = run_plan(eng, arena, off, ln, idx, first, launches=0)
    want_req = want_batch(arena, off, ln)
    assert np.array_equal(req, want_req)
    assert np.array_equal(bat, rows([H(r.tobytes()) for r in want_req]))


# calls above the launchers ----------------------------------------------------
@pytest.fixture(scope="module")
def small_cycle():
    rng = np.random.default_rng(14)
    msgs = [rng.integers(0, 256, size=33, dtype=np.uint8).tobytes() for _ in range(16)]
    return msgs, [[m[:7], m[7:]] for m in msgs], [H(m) for m in msgs]


def test_hash_verify_and_ring_calls_follow_the_route(eng, small_cycle):
    msgs, reqs, want = small_cycle
    with Route(eng, 1):
        assert np.array_equal(eng.hash_slices(reqs), rows(want))
    expected = list(want)
    expected[11] = bytes(32)
    with Route(eng, 1):
        assert eng.verify_slices(reqs, expected).tolist() == [11]
    with Route(eng, 1):
        ticket = eng.submit_slices(reqs + reqs[:5], dedup=True)
        assert np.array_equal(eng.wait(ticket), rows(want + want[:5]))


def test_the_default_hasher_never_counts(own, small_cycle):
    msgs, reqs, _ = small_cycle
    own.set_hasher("sha256")
    with Route(own, 0):
        got = own.hash_slices(reqs)
    assert np.array_equal(got, rows([hashlib.sha256(m).digest() for m in msgs]))
