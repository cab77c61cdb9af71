"""Checkpoint chains under SHA-512/256 (mirsha_chains_create_hasher and the
kernels of mirsha_sha512_chains.hip): the device form of the testengine log's
ActiveHash (testengine/recorder.go:186-256) when the node's Hasher is
sha512.New512_256.  Expected values come from hashlib streaming hashers, one
per chain; never from the code under test.  The shapes are the smallest at
which each path can go wrong: every count of pending digests (four fill a
128-byte block) against every count of writes before, between and after
checkpoints, wave edges, segments of one chain in two waves."""
import ctypes
import hashlib

import numpy as np
import pytest

from mirbft_amd import (HASHERS, Actions, Checkpoint, CheckpointChains, Commit, CommitBatch, DeviceLog, Engine,
                        HashRequest, MirshaError, Processor, ProcessorWorkPool, _lib, commit_plan)

pytestmark = pytest.mark.gpu

NULL = _lib.MIRSHA_NULL_INDEX
CP = _lib.MIRSHA_COMMIT_CHECKPOINT
EMPTY = bytes.fromhex("c672b8d1ef56ed28ab87c3622c5114069bdd3ad7b8f9737498d0c01ecef0967a")


def new(name="sha512_256"):
    return hashlib.new(name)


def H(b) -> bytes:
    return hashlib.new("sha512_256", bytes(b)).digest()


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
    yield own
    own.set_hasher("sha256")


def table_of(rng, m):
    return rng.integers(0, 256, (m, 32), dtype=np.uint8)


def run_ref(ref, table, op_chain, op_digest, name="sha512_256"):
    """The programme on hashlib hashers ref[chain]; returns the checkpoint values in op order."""
    out = []
    for c, d in zip(op_chain, op_digest):
        c, d = int(c), int(d)
        if d == NULL:
            continue
        if d == CP:
            out.append(ref[c].digest())
            ref[c] = new(name)
        else:
            ref[c].update(table[d].tobytes())
    return out


def sums(ch, which=None):
    which = np.arange(ch.n, dtype=np.uint32) if which is None else which
    return [g.tobytes() for g in ch.sum(which)]


def values(got):
    return [g.tobytes() for g in got]


def interleave(rng, programmes):
    """[(chain, [op_digest...])] -> (op_chain, op_digest) in a random
    interleaving that keeps every chain's own order."""
    owner = np.concatenate([np.full(len(p), k, dtype=np.int64) for k, (_, p) in enumerate(programmes)] or
                           [np.empty(0, dtype=np.int64)])
    rng.shuffle(owner)
    at = [0] * len(programmes)
    oc, od = [], []
    for k in owner:
        chain, prog = programmes[k]
        oc.append(chain)
        od.append(prog[at[k]])
        at[k] += 1
    return np.asarray(oc, dtype=np.uint32), np.asarray(od, dtype=np.uint32)


def random_cycle(rng, n, n_ops, n_digests):
    oc = rng.integers(0, n, n_ops).astype(np.uint32)
    od = rng.integers(0, n_digests, n_ops).astype(np.uint32)
    kind = rng.random(n_ops)
    od[kind < 0.1] = NULL
    od[kind > 0.9] = CP
    return oc, od


# ---- 1. parity classes --------------------------------------------------------------------

ALL = [(p, a, m, b) for p in range(4) for a in range(6) for m in [None] + list(range(6)) for b in range(6)]
ALONE = [(p, a, m, b) for p in range(4) for a in range(5) for m in (None, 0, 3, 4) for b in range(5)]


@pytest.mark.parametrize("together", [True, False], ids=["one_call", "one_call_per_chain"])
def test_parity_classes(eng, together):
    """(digests pending on entry, writes before the first checkpoint, writes
    between two checkpoints or None for a single one, writes after the last):
    as the lanes of ONE call, and a subset each as a lone lane in a call of its
    own.  The leftover state is checked by a later sum, and again after one
    more write."""
    assert len(ALL) == 1008 and len(ALONE) == 400
    rng = np.random.default_rng(521 + together)
    classes = ALL if together else ALONE
    n = len(classes)
    ch = CheckpointChains(eng, n)
    assert ch.hasher == "sha512_256"
    ref = [new() for _ in range(n)]
    table = table_of(rng, 16)
    pre_chain = np.asarray([c for c, cl in enumerate(classes) for _ in range(cl[0])], dtype=np.uint32)
    pre = table_of(rng, pre_chain.size)
    ch.write(pre, pre_chain)  # the pending digests of an earlier call
    for row, c in zip(pre, pre_chain):
        ref[c].update(row.tobytes())
    w = lambda k: [int(x) for x in rng.integers(0, 16, k)]
    programmes = [(c, w(a) + [CP] + ([] if m is None else w(m) + [CP]) + w(b)) for c, (_, a, m, b) in enumerate(classes)]
    calls = [interleave(rng, programmes)] if together else [interleave(rng, [p]) for p in programmes]
    got, want = [], []
    for oc, od in calls:
        got += values(ch.commit(table, oc, od))
        want += run_ref(ref, table, oc, od)
    assert got == want
    assert sums(ch) == [r.digest() for r in ref]
    more = table_of(rng, n)
    ch.write(more, np.arange(n, dtype=np.uint32))
    for row, r in zip(more, ref):
        r.update(row.tobytes())
    assert sums(ch) == [r.digest() for r in ref]
    ch.close()


# ---- 2. empty checkpoints -----------------------------------------------------------------

def test_empty_checkpoints(eng):
    rng = np.random.default_rng(522)
    table = table_of(rng, 3)
    ch = CheckpointChains(eng, 3)
    assert hashlib.new("sha512_256", b"").digest() == EMPTY
    # the very first op on a fresh chain, and two back to back
    got = values(ch.commit(table, [0, 1, 1, 1], [CP, 0, CP, CP]))
    assert got == [EMPTY, H(table[0].tobytes()), EMPTY]
    assert sums(ch) == [EMPTY] * 3
    # a checkpoint as the last op: the next call starts the chain empty
    assert values(ch.commit(table, [2, 2, 2], [1, 2, CP])) == [H(table[1].tobytes() + table[2].tobytes())]
    assert values(ch.commit(table, [2, 2], [0, CP])) == [H(table[0].tobytes())]
    assert values(ch.commit(table, [2], [CP])) == [EMPTY]
    # an empty table: checkpoints and nulls only
    assert values(ch.commit(np.zeros((0, 32), np.uint8), [0, 0, 1], [NULL, CP, CP])) == [EMPTY, EMPTY]
    assert ch.commit(table, [], []).shape == (0, 32)
    assert sums(ch) == [EMPTY] * 3
    ch.close()


# ---- 3. widths ----------------------------------------------------------------------------

@pytest.mark.parametrize("n_active", [1, 63, 64, 65, 257])
def test_widths(eng, n_active):
    """n_active chains with entries in one call (that many lanes): 1 to 40 ops
    each, 0-3 checkpoints among them, any count of pending digests.  Between
    them idle chains, at least one in every 64 ids and so in every wave's
    range, with a state of their own that must not change."""
    rng = np.random.default_rng(5300 + n_active)
    n = n_active + n_active // 50 + 2
    idle = set(range(7, n, 50)) | {n - 1}
    active = [c for c in range(n) if c not in idle][:n_active]
    idle = [c for c in range(n) if c not in active]
    assert len(active) == n_active and idle
    assert all(any(c in idle for c in range(lo, min(lo + 64, n))) for lo in range(0, n, 64))
    ch = CheckpointChains(eng, n)
    ref = [new() for _ in range(n)]
    pre_chain = np.asarray([c for c in range(n) for _ in range(int(rng.integers(0, 6)) if c not in idle else 1 + c % 3)],
                           dtype=np.uint32)
    rng.shuffle(pre_chain)
    pre = table_of(rng, pre_chain.size)
    ch.write(pre, pre_chain)
    for row, c in zip(pre, pre_chain):
        ref[c].update(row.tobytes())
    idle_before = sums(ch, np.asarray(idle, dtype=np.uint32))
    assert idle_before == [ref[c].digest() for c in idle]
    table = table_of(rng, 97)
    programmes = []
    for k, c in enumerate(active):
        length = 1 + (k * 7) % 40 if n_active > 1 else 40
        prog = [int(x) for x in rng.integers(0, 97, length)]
        for at in rng.integers(0, length, int(rng.integers(0, 4))):
            prog[int(at)] = CP
        if length >= 3:  # at most two nulls: an entry is left
            for at in rng.integers(0, length, 2):
                if prog[int(at)] != CP and rng.random() < 0.5:
                    prog[int(at)] = NULL
        programmes.append((c, prog))
    programmes.append((idle[0], [NULL, NULL]))
    oc, od = interleave(rng, programmes)
    act, _, _, n_values = commit_plan(oc, od, n, 97)
    assert act.tolist() == active and n_values == int(np.count_nonzero(od == CP))
    assert values(ch.commit(table, oc, od)) == run_ref(ref, table, oc, od)
    assert sums(ch, np.asarray(idle, dtype=np.uint32)) == idle_before
    assert sums(ch) == [r.digest() for r in ref]
    ch.close()


# ---- 4. equivalence of the calls on one object --------------------------------------------

def old_calls(ch, table, oc, od):
    """The programme through write / sum / reset, cut at every checkpoint."""
    out = []
    pend_d, pend_c = [], []

    def flush():
        if pend_d:
            ch.write(table[np.asarray(pend_d)], np.asarray(pend_c, dtype=np.uint32))
            pend_d.clear()
            pend_c.clear()

    for c, d in zip(oc, od):
        c, d = int(c), int(d)
        if d == NULL:
            continue
        if d == CP:
            flush()
            out.append(ch.sum([c])[0].tobytes())
            ch.reset([c])
        else:
            pend_d.append(d)
            pend_c.append(c)
    flush()
    return out


def test_equivalence_with_write_sum_reset(eng):
    rng = np.random.default_rng(524)
    n = 70
    a, b, mixed = (CheckpointChains(eng, n) for _ in range(3))
    ref = [new() for _ in range(n)]
    for cycle in range(4):
        table = table_of(rng, 50)
        oc, od = random_cycle(rng, n, int(rng.integers(100, 400)), 50)
        want = run_ref(ref, table, oc, od)
        assert values(a.commit(table, oc, od)) == want, cycle
        assert old_calls(b, table, oc, od) == want, cycle
        # one object, the two forms in turn
        form = values(mixed.commit(table, oc, od)) if cycle % 2 else old_calls(mixed, table, oc, od)
        assert form == want, cycle
        final = [r.digest() for r in ref]
        assert sums(a) == final and sums(b) == final and sums(mixed) == final, cycle
    for ch in (a, b, mixed):
        ch.close()


# ---- 5. the device form -------------------------------------------------------------------

def test_commit_device_on_hashed_requests(eng):
    """Request digests written by hash_batch_device under SHA-512/256 into a
    torch buffer are committed where they lie."""
    import torch

    rng = np.random.default_rng(525)
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
    dev, hst = CheckpointChains(eng, n), CheckpointChains(eng, n)
    ref = [new() for _ in range(n)]
    got = values(dev.commit_device(d_out.data_ptr(), n_req, oc, od))  # queued behind the hashing
    want = run_ref(ref, host, oc, od)
    assert got == want and len(want) > 10
    assert values(hst.commit(host, oc, od)) == want
    assert sums(dev) == sums(hst) == [r.digest() for r in ref]
    assert np.array_equal(d_out.cpu().numpy(), host)
    dev.close()
    hst.close()


# ---- 6. the ring --------------------------------------------------------------------------

def cycle_with_checkpoints(rng, n, per_chain, n_digests, k_cp):
    """Every chain: k_cp stretches of per_chain writes, each closed by a checkpoint, then two writes."""
    programmes = []
    for c in range(n):
        prog = []
        for _ in range(k_cp):
            prog += [int(x) for x in rng.integers(0, n_digests, per_chain)] + [CP]
        programmes.append((c, prog + [int(x) for x in rng.integers(0, n_digests, 2)]))
    return interleave(rng, programmes)


def test_ring_tickets(eng):
    rng = np.random.default_rng(526)
    n = 3
    ch = CheckpointChains(eng, n)
    ref = [new() for _ in range(n)]
    table = table_of(rng, 40)
    # digests pending from an earlier call: 1, 2 and 3 of them
    pre_chain = np.asarray([0, 1, 1, 2, 2, 2], dtype=np.uint32)
    ch.write(table[:6], pre_chain)
    for row, c in zip(table[:6], pre_chain):
        ref[c].update(row.tobytes())
    # one checkpoint a chain into a pageable out, four into page-locked memory
    oc, od = cycle_with_checkpoints(rng, n, 5, 40, 1)
    out = np.zeros((n, 32), dtype=np.uint8)
    t = ch.submit_commit(table, oc, od, out=out)
    assert t.values is out
    assert values(eng.wait(t)) == run_ref(ref, table, oc, od)
    oc, od = cycle_with_checkpoints(rng, n, 6, 40, 4)
    pinned = eng.host_empty(32 * 4 * n).reshape(-1, 32)
    pinned[:] = 0
    t = ch.submit_commit(table, oc, od, out=pinned)
    assert values(eng.wait(t)) == run_ref(ref, table, oc, od)
    assert sums(ch) == [r.digest() for r in ref]
    # chain 0 with 70 checkpoints beside two others: its FIRST and its LAST
    # segment lie in different waves, so FIRST lanes read the states' snapshot
    programmes = [(0, sum(([int(x) for x in rng.integers(0, 40, k % 6)] + [CP] for k in range(70)), []) + [7, 8, 9]),
                  (1, [1, 2, 3, CP, 4]), (2, [5])]
    oc, od = interleave(rng, programmes)
    assert sums(ch) != [EMPTY] * n  # pending rows and midstates that the snapshot has to carry
    t = ch.submit_commit(table, oc, od)
    assert values(eng.wait(t)) == run_ref(ref, table, oc, od)
    assert sums(ch) == [r.digest() for r in ref]
    # two tickets back to back, collected in reverse order
    tickets, want = [], []
    for _ in range(2):
        oc, od = random_cycle(rng, n, 120, 40)
        tickets.append(ch.submit_commit(table, oc, od))
        want.append(run_ref(ref, table, oc, od))
    assert tickets[1].value == tickets[0].value + 1
    assert values(eng.wait(tickets[1])) == want[1] and values(eng.wait(tickets[0])) == want[0]
    # a commit ticket beside a hashing ticket, then a synchronous commit that orders behind the ticket
    reqs = [[rng.bytes(int(k)) for k in rng.integers(0, 200, 2)] for _ in range(70)]
    hashing = eng.submit_slices(reqs)
    oc, od = random_cycle(rng, n, 200, 40)
    commit = ch.submit_commit(table, oc, od)
    want_commit = run_ref(ref, table, oc, od)
    oc2, od2 = random_cycle(rng, n, 60, 40)
    assert values(ch.commit(table, oc2, od2)) == run_ref(ref, table, oc2, od2)
    assert values(eng.wait(commit)) == want_commit
    assert values(eng.wait(hashing)) == [H(b"".join(r)) for r in reqs]
    assert sums(ch) == [r.digest() for r in ref]
    ch.close()


# ---- 7. refusals --------------------------------------------------------------------------

def test_refusals_name_both_hashers_and_change_nothing(own):
    rng = np.random.default_rng(527)
    table = table_of(rng, 8)
    oc, od = [0, 0, 1, 0, 1], [0, 1, 2, CP, 3]
    lib = own._lib
    try:
        for mine, other in (("sha512_256", "sha256"), ("sha256", "sha512_256")):
            own.set_hasher(mine)
            ch = CheckpointChains(own, 2)  # takes the engine's hasher
            assert ch.hasher == mine and lib.mirsha_chains_hasher(ch.handle) == HASHERS[mine]
            ref = [new(mine) for _ in range(2)]
            ch.write(table[4:7], [0, 1, 1])
            for row, c in zip(table[4:7], [0, 1, 1]):
                ref[c].update(row.tobytes())
            before = sums(ch)
            assert before == [r.digest() for r in ref]
            first = own.submit_slices([[b"a"]])
            own.wait(first)
            own.set_hasher(other)
            for refused in (lambda: ch.write(table[:1], [0]), lambda: ch.sum([0]),
                            lambda: ch.commit(table, oc, od), lambda: ch.submit_commit(table, oc, od)):
                with pytest.raises(MirshaError) as ei:
                    refused()
                assert ei.value.code == _lib.MIRSHA_EINVAL, str(ei.value)
                assert "sha256" in str(ei.value).replace("sha512_256", "") and "sha512_256" in str(ei.value), str(ei.value)
            after = own.submit_slices([[b"a"]])
            own.wait(after)
            assert after.value == first.value + 1  # the refused submission took no ticket
            own.set_hasher(mine)
            assert sums(ch) == before
            assert values(ch.commit(table, oc, od)) == run_ref(ref, table, oc, od, mine)
            assert sums(ch) == [r.digest() for r in ref]
            # reset hashes nothing: served under either context, to the H0 of the chains' own hasher
            own.set_hasher(other)
            ch.reset([1])
            own.set_hasher(mine)
            assert sums(ch) == [ref[0].digest(), new(mine).digest()]
            ch.close()
        # an unknown hasher; and mirsha_chains_create yields SHA-256 chains whatever the context's hasher
        own.set_hasher("sha512_256")
        h = ctypes.c_void_p()
        assert lib.mirsha_chains_create_hasher(own.ctx, 2, 7, ctypes.byref(h)) == _lib.MIRSHA_EINVAL and not h.value
        with pytest.raises(ValueError):
            CheckpointChains(own, 2, hasher="sha3")
        assert lib.mirsha_chains_create(own.ctx, 2, ctypes.byref(h)) == _lib.MIRSHA_OK
        assert lib.mirsha_chains_hasher(h) == _lib.MIRSHA_HASHER_SHA256
        lib.mirsha_chains_destroy(h)
        explicit = CheckpointChains(own, 2, hasher="sha256")
        assert explicit.hasher == "sha256"
        explicit.close()
    finally:
        own.set_hasher("sha256")


# ---- 8. Processor level -------------------------------------------------------------------

class NodeState:
    """testengine's application state restated (recorder.go:186-256) with the node's Hasher."""

    def __init__(self):
        self.active = new()

    def commit(self, commits):
        out = []
        for c in commits:
            if c.batch is not None:
                for d in c.batch.digests:
                    self.active.update(d or b"")
            else:
                out.append(self.active.digest())
                self.active = new()
        return out


@pytest.mark.parametrize("async_commits", [False, True], ids=["sync", "async_commits"])
@pytest.mark.parametrize("cls", [Processor, ProcessorWorkPool])
def test_processor_with_a_device_log(own, cls, async_commits):
    rng = np.random.default_rng(528)
    own.set_hasher("sha256")
    early = DeviceLog(own, n_nodes=4)  # made before the hasher is set: SHA-256 chains
    try:
        p = cls(engine=own, hasher="sha512_256", async_commits=async_commits)
        log = DeviceLog(own, n_nodes=4, node=1)
        assert log.chains.hasher == "sha512_256" and early.chains.hasher == "sha256"
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
                if seq % 3 == 0:  # a checkpoint in the middle of the list
                    commits.append(Commit(checkpoint=Checkpoint(seq_no=seq)))
            actions = Actions(hash=reqs, commits=commits)
            res = p.submit(actions).wait() if (async_commits and cls is Processor) else p.process(actions)
            assert [r.digest for r in res.digests] == [H(b"".join(q.data)) for q in reqs]
            asked = [c for c in commits if c.checkpoint is not None]
            assert [r.value for r in res.checkpoints] == state.commit(commits)
            assert [r.commit for r in res.checkpoints] == asked
            for node in range(4):  # every node's chain holds the same value
                assert [v.tobytes() for v in log.values[:, node]] == [r.value for r in res.checkpoints]
        assert sums(log.chains) == [state.active.digest()] * 4
        p.log = early
        with pytest.raises(MirshaError) as ei:
            p.process(Actions(hash=[HashRequest(data=[b"x"], origin=0)],
                              commits=[Commit(batch=CommitBatch([rng.bytes(32)], seq_no=1))]))
        assert ei.value.code == _lib.MIRSHA_EINVAL
        log.close()
    finally:
        own.set_hasher("sha256")
        early.close()


# ---- 9. the C++ mirror --------------------------------------------------------------------

@pytest.mark.parametrize("flags", [8, 8 | 2, 8 | 4], ids=["process", "submit_wait", "async_commits"])
def test_cpp_host_mirror_commit_loop(flags):
    rng = np.random.default_rng(529)
    host = ctypes.CDLL(_lib.HOST_LIB_PATH)
    assert host.mirbft_host_features() & 2  # this build knows the flag (an older one would ignore it)
    batch_len = [3, 0, 0xFFFFFFFF, 0xFFFFFFFF, 5, 1, 0xFFFFFFFF, 2]  # 5 batches, 3 checkpoints
    rows = [None if k in (1, 6) else rng.bytes(32) for k in range(11)]
    bufs = [ctypes.create_string_buffer(r, 32) if r is not None else None for r in rows]
    ptrs = (ctypes.c_void_p * len(rows))(*[ctypes.addressof(b) if b is not None else None for b in bufs])
    lens = (ctypes.c_uint32 * len(batch_len))(*batch_len)
    n_nodes = 4
    out = (ctypes.c_uint8 * (32 * 3 * n_nodes))()
    k = ctypes.c_uint32(0)
    err = ctypes.create_string_buffer(256)
    host.mirbft_host_commit.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                        ctypes.c_char_p, ctypes.c_uint32]
    rc = host.mirbft_host_commit(0, n_nodes, ptrs, lens, len(batch_len), out, ctypes.byref(k), flags, err, 256)
    assert rc == 0, err.value
    state, want, at = new(), [], 0
    for m in batch_len:
        if m == 0xFFFFFFFF:
            want.append(state.digest())
            state = new()
        else:
            for r in rows[at:at + m]:
                state.update(r or b"")
            at += m
    assert k.value == 3 and want[1] == EMPTY
    got = [bytes(out[32 * i:32 * i + 32]) for i in range(3 * n_nodes)]
    assert got == [w for w in want for _ in range(n_nodes)]
