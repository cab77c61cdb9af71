"""The producer/consumer pair route of the SHA-512/256 checkpoint chains on the
device (mirsha_sha512_chains_pair.hip): the commit launches of calls and
tickets split the walk of a chain's entries and the rounds over two waves.
Against hashlib streaming hashers, one per chain, bit-exact; every case also
asserts the route by the change of CheckpointChains.pair_launches (+1 for each
launch that must take a pair kernel, +0 where the one-lane kernels must run)
and a canary behind the output rows.  The shapes are the smallest at which the
pair kernels can still go wrong: every class of step in one wave with lanes of
different lengths, a long lane beside finished ones, partial groups and several
workgroups with idle chains in between, the routes in turn on one object,
tickets whose segments straddle groups, and both sides of the threshold, which
is read from the library."""
import hashlib

import numpy as np
import pytest

from mirbft_amd import (Actions, Checkpoint, CheckpointChains, Commit, CommitBatch, DeviceLog, Engine, HashRequest,
                        Processor, sha512_pair_max_groups)
from test_gpu_sha512_chains import (CP, EMPTY, NULL, H, NodeState, cycle_with_checkpoints, interleave, new,
                                    random_cycle, run_ref, sums, table_of, values)

pytestmark = pytest.mark.gpu
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
    own.set_variant(0)
    yield own
    own.set_variant(0)
    own.set_hasher("sha256")


class Route:
    """with Route(chains, k): the block queues exactly k pair launches on the chains."""

    def __init__(self, ch, launches):
        self.ch, self.launches = ch, launches

    def __enter__(self):
        self.before = self.ch.pair_launches

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            got = self.ch.pair_launches - self.before
            assert got == self.launches, f"{got} pair launches, {self.launches} expected"


def rows_out(n, eng=None):
    """(the (n, 32) array a call writes, the canary rows behind it); page-locked with ``eng``."""
    big = (eng.host_empty(32 * (n + 4)) if eng is not None else np.empty(32 * (n + 4), dtype=np.uint8)).reshape(-1, 32)
    big[:] = CANARY
    return big[:n], big[n:]


def commit(ch, table, oc, od):
    """ch.commit into canaried rows; the values as bytes."""
    n = int(np.count_nonzero(np.asarray(od, dtype=np.uint32) == CP))
    out, behind = rows_out(n)
    got = ch.commit(table, oc, od, out=out)
    assert got is out and (behind == CANARY).all()
    return values(got)


def absorb(ch, ref, rows, chain_of):
    ch.write(rows, chain_of)
    for row, c in zip(rows, chain_of):
        ref[int(c)].update(row.tobytes())


def digests_of(ref):
    return [r.digest() for r in ref]


# ---- step classes --------------------------------------------------------------------------

def test_every_step_class_in_one_launch(eng):
    """64 chains in one group; chain c enters with c % 4 pending digests and
    visits a full block, a checkpoint after 0..3 writes (with and without
    pending rows), two checkpoints in a row and an end with 1-3 writes left
    pending.  The programmes differ in length, so lanes finish at different
    steps."""
    rng = np.random.default_rng(5401)
    n = 64
    ch = CheckpointChains(eng, n)
    ref = [new() for _ in range(n)]
    pre_chain = np.asarray([c for c in range(n) for _ in range(c % 4)], dtype=np.uint32)
    with Route(ch, 1):  # a programme of writes
        absorb(ch, ref, table_of(rng, pre_chain.size), pre_chain)
    table = table_of(rng, 32)
    w = lambda k: [int(x) for x in rng.integers(0, 32, k)]
    programmes = []
    for c in range(n):
        p = c % 4
        prog = w((c // 4) % 4) + [CP]  # a checkpoint after 0..3 writes on top of p pending rows
        prog += w(4 - p if c % 8 < 4 else 4)  # a full block
        for j in range(4):
            prog += w(j) + [CP]  # from an empty message: after 0..3 writes
        prog += w(2 * (c % 7)) + [CP, CP]  # lengths differ; two checkpoints in a row
        prog += w(1 + c % 3)  # 1-3 writes left pending
        programmes.append((c, prog))
    assert len({len(p) for _, p in programmes}) > 10
    oc, od = interleave(rng, programmes)
    with Route(ch, 1):
        got = commit(ch, table, oc, od)
    assert got == run_ref(ref, table, oc, od)
    assert sums(ch) == digests_of(ref)
    # the pending rows it left are the next call's first slots
    more = table_of(rng, n)
    with Route(ch, 1):
        absorb(ch, ref, more, np.arange(n, dtype=np.uint32))
    assert sums(ch) == digests_of(ref)
    ch.close()


def test_a_long_lane_beside_finished_ones(eng):
    rng = np.random.default_rng(5402)
    n = 64
    ch = CheckpointChains(eng, n)
    ref = [new() for _ in range(n)]
    table = table_of(rng, 50)
    programmes = []
    for c in range(n):
        prog = [int(x) for x in rng.integers(0, 50, int(rng.integers(0, 6)))]
        if c == 17:
            prog = [int(x) for x in rng.integers(0, 50, 400)]
            for at in (90, 91, 333):
                prog.insert(at, CP)
        elif prog and rng.random() < 0.3:
            prog[int(rng.integers(0, len(prog)))] = CP
        programmes.append((c, prog))
    oc, od = interleave(rng, programmes)
    with Route(ch, 1):
        got = commit(ch, table, oc, od)
    assert got == run_ref(ref, table, oc, od)
    assert sums(ch) == digests_of(ref)
    ch.close()


# ---- widths --------------------------------------------------------------------------------

@pytest.mark.parametrize("n_active", [1, 63, 64, 65, 257])
def test_widths(eng, n_active):
    """n_active lanes: partial groups and several workgroups.  Between the
    active chains lie idle ones, at least one in every 64 ids, with a state of
    their own (from an earlier absorb) that must not change."""
    rng = np.random.default_rng(5410 + n_active)
    n = n_active + n_active // 50 + 2
    idle = set(range(7, n, 50)) | {n - 1}
    active = [c for c in range(n) if c not in idle][:n_active]
    idle = [c for c in range(n) if c not in active]
    assert len(active) == n_active and idle
    ch = CheckpointChains(eng, n)
    ref = [new() for _ in range(n)]
    pre_chain = np.asarray([c for c in range(n) for _ in range(int(rng.integers(0, 6)) if c in active else 1 + c % 3)],
                           dtype=np.uint32)
    rng.shuffle(pre_chain)
    absorb(ch, ref, table_of(rng, pre_chain.size), pre_chain)
    idle_ids = np.asarray(idle, dtype=np.uint32)
    idle_before = sums(ch, idle_ids)
    assert idle_before == [ref[c].digest() for c in idle]
    table = table_of(rng, 97)
    programmes = []
    for k, c in enumerate(active):
        length = 1 + (k * 7) % 40 if n_active > 1 else 40
        prog = [int(x) for x in rng.integers(0, 97, length)]
        for at in rng.integers(0, length, int(rng.integers(0, 4))):
            prog[int(at)] = CP
        if length >= 3 and rng.random() < 0.5:
            at = int(rng.integers(0, length))
            prog[at] = NULL if prog[at] != CP else CP
        programmes.append((c, prog))
    programmes = [(c, p) for c, p in programmes if any(d != NULL for d in p)]
    oc, od = interleave(rng, programmes)
    assert len(programmes) == n_active
    with Route(ch, 1):
        got = commit(ch, table, oc, od)
    assert got == run_ref(ref, table, oc, od)
    assert sums(ch, idle_ids) == idle_before
    assert sums(ch) == digests_of(ref)
    ch.close()


# ---- the routes in turn on one object ------------------------------------------------------

def test_routes_interchange_on_one_object(eng):
    rng = np.random.default_rng(5420)
    n = 70
    ch = CheckpointChains(eng, n)
    ref = [new() for _ in range(n)]
    table = table_of(rng, 50)

    def one_commit(launches):
        oc, od = random_cycle(rng, n, int(rng.integers(150, 400)), 50)
        with Route(ch, launches):
            got = commit(ch, table, oc, od)
        assert got == run_ref(ref, table, oc, od)
        assert sums(ch) == digests_of(ref)

    try:
        eng.set_variant(6)
        one_commit(1)
        eng.set_variant(5)
        one_commit(0)
        eng.set_variant(0)
        rows = table_of(rng, 200)
        with Route(ch, 1):
            absorb(ch, ref, rows, rng.integers(0, n, 200).astype(np.uint32))
        with Route(ch, 0):
            assert sums(ch) == digests_of(ref)
            which = np.asarray([3, 64, 69], dtype=np.uint32)
            ch.reset(which)
        for c in which:
            ref[int(c)] = new()
        assert sums(ch) == digests_of(ref)
        one_commit(1)
    finally:
        eng.set_variant(0)
    ch.close()


# ---- tickets -------------------------------------------------------------------------------

@pytest.mark.parametrize("pinned", [True, False], ids=["page_locked", "pageable"])
def test_ticket_with_four_checkpoints_a_chain(eng, pinned):
    """64 chains, five segments each: 320 lanes in five groups."""
    rng = np.random.default_rng(5430 + pinned)
    n = 64
    ch = CheckpointChains(eng, n)
    ref = [new() for _ in range(n)]
    table = table_of(rng, 40)
    pre_chain = np.asarray([c for c in range(n) for _ in range(c % 4)], dtype=np.uint32)
    absorb(ch, ref, table_of(rng, pre_chain.size), pre_chain)
    oc, od = cycle_with_checkpoints(rng, n, 6, 40, 4)
    out, behind = rows_out(4 * n, eng if pinned else None)
    with Route(ch, 1):
        t = ch.submit_commit(table, oc, od, out=out)
        got = eng.wait(t)
    assert got is out and (behind == CANARY).all()
    assert values(got) == run_ref(ref, table, oc, od)
    assert sums(ch) == digests_of(ref)
    ch.close()


def test_ticket_whose_first_and_last_segment_lie_in_different_groups(eng):
    """Chain 0 with 70 checkpoints beside two others: more than 64 segments, so
    FIRST lanes read the states' snapshot; the chains enter with pending rows
    and midstates that the snapshot has to carry."""
    rng = np.random.default_rng(5432)
    n = 3
    ch = CheckpointChains(eng, n)
    ref = [new() for _ in range(n)]
    table = table_of(rng, 40)
    pre_chain = np.asarray([0] * 5 + [1] * 2 + [2] * 7, dtype=np.uint32)
    absorb(ch, ref, table_of(rng, pre_chain.size), pre_chain)
    assert sums(ch) != [EMPTY] * n
    programmes = [(0, sum(([int(x) for x in rng.integers(0, 40, k % 6)] + [CP] for k in range(70)), []) + [7, 8, 9]),
                  (1, [1, 2, 3, CP, 4]), (2, [5])]
    oc, od = interleave(rng, programmes)
    out, behind = rows_out(71, eng)
    with Route(ch, 1):
        t = ch.submit_commit(table, oc, od, out=out)
        got = eng.wait(t)
    assert (behind == CANARY).all()
    assert values(got) == run_ref(ref, table, oc, od)
    assert sums(ch) == digests_of(ref)
    ch.close()


def test_ticket_beside_a_hashing_ticket(eng):
    rng = np.random.default_rng(5433)
    n = 5
    ch = CheckpointChains(eng, n)
    ref = [new() for _ in range(n)]
    table = table_of(rng, 40)
    reqs = [[rng.bytes(int(k)) for k in rng.integers(0, 200, 2)] for _ in range(70)]
    hashing = eng.submit_slices(reqs)
    oc, od = random_cycle(rng, n, 200, 40)
    out, behind = rows_out(int(np.count_nonzero(od == CP)))
    with Route(ch, 1):
        t = ch.submit_commit(table, oc, od, out=out)
    want = run_ref(ref, table, oc, od)
    oc2, od2 = random_cycle(rng, n, 60, 40)
    with Route(ch, 1):  # a synchronous commit orders behind the ticket
        assert commit(ch, table, oc2, od2) == run_ref(ref, table, oc2, od2)
    assert values(eng.wait(t)) == want and (behind == CANARY).all()
    assert values(eng.wait(hashing)) == [H(b"".join(r)) for r in reqs]
    assert sums(ch) == digests_of(ref)
    ch.close()


# ---- the device form -----------------------------------------------------------------------

def test_commit_device_on_hashed_requests(eng):
    import torch

    rng = np.random.default_rng(5440)
    n_req, n = 100, 5
    ln = rng.integers(0, 300, n_req).astype(np.uint32)
    off = np.zeros(n_req, dtype=np.uint64)
    np.cumsum(ln[:-1].astype(np.uint64), out=off[1:])
    arena = rng.integers(0, 256, int(ln.sum()) + 1, dtype=np.uint8)
    host = np.frombuffer(b"".join(H(arena[int(o):int(o) + int(k)].tobytes()) for o, k in zip(off, ln)),
                         dtype=np.uint8).reshape(n_req, 32)
    d_arena = torch.from_numpy(arena).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_len = torch.from_numpy(ln.view(np.int32)).cuda()
    d_out = torch.zeros((n_req, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.hash_batch_device(d_arena.data_ptr(), arena.size, d_off.data_ptr(), d_len.data_ptr(), None, n_req,
                          d_out.data_ptr())
    oc, od = random_cycle(rng, n, 300, n_req)
    ch = CheckpointChains(eng, n)
    ref = [new() for _ in range(n)]
    out, behind = rows_out(int(np.count_nonzero(od == CP)))
    with Route(ch, 1):
        got = ch.commit_device(d_out.data_ptr(), n_req, oc, od, out=out)  # queued behind the hashing
    want = run_ref(ref, host, oc, od)
    assert values(got) == want and len(want) > 10 and (behind == CANARY).all()
    assert sums(ch) == digests_of(ref)
    assert np.array_equal(d_out.cpu().numpy(), host)
    ch.close()


# ---- the threshold -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def threshold_cycle():
    """One chain more than the largest launch that takes the pair: a write and
    a checkpoint each.  The reference is computed once."""
    n = 64 * sha512_pair_max_groups() + 1
    rng = np.random.default_rng(5450)
    table = table_of(rng, 16)
    row_hash = [H(r.tobytes()) for r in table]
    oc = np.repeat(np.arange(n, dtype=np.uint32), 2)
    od = np.empty(2 * n, dtype=np.uint32)
    od[0::2] = rng.integers(0, 16, n)
    od[1::2] = CP
    return n, table, oc, od, [row_hash[int(d)] for d in od[0::2]]


def one_write_and_a_checkpoint(eng, cycle, lanes, launches):
    n, table, oc, od, want = cycle
    ch = CheckpointChains(eng, n)
    with Route(ch, launches):
        got = commit(ch, table, oc[: 2 * lanes], od[: 2 * lanes])
    assert got == want[:lanes]
    probe = np.asarray([0, lanes - 1, n - 1], dtype=np.uint32)
    assert sums(ch, probe) == [EMPTY] * 3
    ch.close()


def test_both_sides_of_the_threshold(eng, threshold_cycle):
    n = threshold_cycle[0]
    if n > 1:
        one_write_and_a_checkpoint(eng, threshold_cycle, n - 1, 1)
    one_write_and_a_checkpoint(eng, threshold_cycle, n, 0)


def test_variants_force_either_kernel(eng, threshold_cycle):
    n = threshold_cycle[0]
    try:
        eng.set_variant(6)
        one_write_and_a_checkpoint(eng, threshold_cycle, n, 1)
        eng.set_variant(5)
        one_write_and_a_checkpoint(eng, threshold_cycle, min(64, n), 0)
    finally:
        eng.set_variant(0)


# ---- the other hasher ----------------------------------------------------------------------

def test_sha256_chains_never_count(own):
    rng = np.random.default_rng(5460)
    own.set_hasher("sha256")
    own.set_variant(0)
    n = 5
    ch = CheckpointChains(own, n, hasher="sha256")
    ref = [hashlib.sha256() for _ in range(n)]
    table = table_of(rng, 40)
    oc, od = random_cycle(rng, n, 200, 40)
    try:
        for variant in (0, 6):
            own.set_variant(variant)
            with Route(ch, 0):
                got = commit(ch, table, oc, od)
                t = ch.submit_commit(table, oc, od)
                again = values(own.wait(t))
            assert got == run_ref(ref, table, oc, od, "sha256")
            assert again == run_ref(ref, table, oc, od, "sha256")
        assert ch.pair_launches == 0
    finally:
        own.set_variant(0)
    ch.close()


# ---- Processor level -----------------------------------------------------------------------

@pytest.mark.parametrize("async_commits", [False, True], ids=["sync", "async_commits"])
def test_processor_with_a_device_log_takes_the_pair(own, async_commits):
    rng = np.random.default_rng(5470)
    own.set_hasher("sha256")
    own.set_variant(0)
    log = None
    try:
        p = Processor(engine=own, hasher="sha512_256", async_commits=async_commits)
        log = DeviceLog(own, n_nodes=4, node=1)
        assert log.chains.hasher == "sha512_256" and log.chains.pair_launches == 0
        p.log = log
        state = NodeState()
        seq = 0
        for cycle in range(3):
            reqs = [HashRequest(data=[rng.bytes(int(k)) for k in rng.integers(0, 90, 3)], origin=i) for i in range(25)]
            commits = []
            for _ in range(7):
                seq += 1
                digests = [None if rng.random() < 0.15 else rng.bytes(32) for _ in range(int(rng.integers(0, 6)))]
                commits.append(Commit(batch=CommitBatch(digests, seq_no=seq)))
                if seq % 3 == 0:
                    commits.append(Commit(checkpoint=Checkpoint(seq_no=seq)))
            actions = Actions(hash=reqs, commits=commits)
            before = log.chains.pair_launches
            res = p.submit(actions).wait() if async_commits else p.process(actions)
            assert [r.digest for r in res.digests] == [H(b"".join(q.data)) for q in reqs]
            assert [r.value for r in res.checkpoints] == state.commit(commits)
            assert log.chains.pair_launches > before
        assert sums(log.chains) == [state.active.digest()] * 4
    finally:
        if log is not None:
            log.close()
        own.set_variant(0)
        own.set_hasher("sha256")
