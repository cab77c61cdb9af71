"""A cycle's Commits as a ticket of the asynchronous ring
(mirsha_chains_commit_submit, one lane per segment between checkpoints): the
commit stage of ProcessorWorkPool beside its hash stage.  Expected values come
from hashlib streaming hashers, one per chain, as NodeState.ActiveHash
(testengine/recorder.go:186-256), and from the golden fixtures; never from the
code under test."""
import ctypes
import hashlib

import numpy as np
import pytest

from mirbft_amd import (Actions, Checkpoint, CheckpointChains, Commit, CommitBatch, CommitTicket, DeviceLog,
                        HashRequest, MirshaError, Processor, ProcessorWorkPool, _lib, commit_seg_plan, hashdata)

pytestmark = pytest.mark.gpu

NULL = _lib.MIRSHA_NULL_INDEX
CP = _lib.MIRSHA_COMMIT_CHECKPOINT
EMPTY = bytes.fromhex("e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855")


def table_of(rng, m):
    return rng.integers(0, 256, (m, 32), dtype=np.uint8)


def run_ref(ref, table, op_chain, op_digest):
    """The programme on hashlib hashers ref[chain]; returns the checkpoint values in op order."""
    out = []
    for c, d in zip(op_chain, op_digest):
        c, d = int(c), int(d)
        if d == NULL:
            continue
        if d == CP:
            out.append(ref[c].digest())
            ref[c] = hashlib.sha256()
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


# ---- 1. parity classes ------------------------------------------------------------------

def parity_classes():
    """tests/test_gpu_commits.py's: (entry parity, writes before the first
    checkpoint, writes between two checkpoints or None for a single
    checkpoint, writes after the last)."""
    return [(odd, a, m, b) for odd in (0, 1) for a in range(4) for m in (None, 0, 1, 2, 3) for b in range(4)]


@pytest.mark.parametrize("together", [True, False], ids=["one_ticket", "one_ticket_per_class"])
def test_parity_classes(engine, together):
    rng = np.random.default_rng(61)
    classes = parity_classes()
    n = len(classes)
    ch = CheckpointChains(engine, n)
    ref = [hashlib.sha256() for _ in range(n)]
    table = table_of(rng, 16)
    odd = [c for c, cl in enumerate(classes) if cl[0]]
    first = table_of(rng, len(odd))
    ch.write(first, np.asarray(odd, dtype=np.uint32))  # the pending digest of an earlier write
    for row, c in zip(first, odd):
        ref[c].update(row.tobytes())
    programmes = []
    for c, (_, a, m, b) in enumerate(classes):
        w = lambda k: [int(x) for x in rng.integers(0, 16, k)]
        programmes.append((c, w(a) + [CP] + ([] if m is None else w(m) + [CP]) + w(b)))
    calls = [interleave(rng, programmes)] if together else [interleave(rng, [p]) for p in programmes]
    tickets = [ch.submit_commit(table, oc, od) for oc, od in calls]  # all queued before any wait
    assert all(isinstance(t, CommitTicket) for t in tickets)
    got, want = [], []
    for t, (oc, od) in zip(tickets, calls):
        v = engine.wait(t)
        assert v is t.values and v.shape == (int(np.count_nonzero(od == CP)), 32)
        got += values(v)
        want += run_ref(ref, table, oc, od)
    assert got == want
    assert sums(ch) == [r.digest() for r in ref]
    more = table_of(rng, n)
    ch.write(more, np.arange(n, dtype=np.uint32))
    for row, r in zip(more, ref):
        r.update(row.tobytes())
    assert sums(ch) == [r.digest() for r in ref]
    ch.close()


# ---- 2. segment widths ------------------------------------------------------------------

WIDTHS = [1, 63, 64, 65, 129, 257]


def check_programme(engine, rng, n, programmes, table, pre=()):
    """Chains ``pre`` get one digest written first (an odd entry parity); the
    programmes run as ONE ticket; values, then every chain's state."""
    ch = CheckpointChains(engine, n)
    ref = [hashlib.sha256() for _ in range(n)]
    if len(pre):
        rows = table_of(rng, len(pre))
        ch.write(rows, np.asarray(pre, dtype=np.uint32))
        for row, c in zip(rows, pre):
            ref[c].update(row.tobytes())
    oc, od = interleave(rng, programmes)
    got = values(engine.wait(ch.submit_commit(table, oc, od)))
    assert got == run_ref(ref, table, oc, od)
    assert sums(ch) == [r.digest() for r in ref]
    ch.close()
    return oc, od


@pytest.mark.parametrize("total", WIDTHS)
def test_widths_one_segment_chains(engine, total):
    rng = np.random.default_rng(600 + total)
    table = table_of(rng, 64)
    programmes = []
    for c in range(total):
        prog = [int(x) for x in rng.integers(0, 64, 1 + (c * 5) % 7)]
        if c % 3 == 0:
            prog.append(CP)  # ends in a checkpoint: still one segment
        programmes.append((c, prog))
    oc, od = check_programme(engine, rng, total + 1, programmes, table, pre=list(range(0, total, 2)))
    assert commit_seg_plan(oc, od, total + 1, 64)[0].size == total


@pytest.mark.parametrize("total", WIDTHS)
@pytest.mark.parametrize("pending", [False, True], ids=["even_entry", "odd_entry"])
def test_widths_one_chain_over_several_waves(engine, total, pending):
    """One chain with total - 1 checkpoints and a trailing write: its first
    segment reads the stored state and its last one stores, waves apart."""
    rng = np.random.default_rng(700 + total)
    table = table_of(rng, 64)
    prog = []
    for k in range(total - 1):
        prog += [int(x) for x in rng.integers(0, 64, k % 4)] + [CP]
    prog.append(int(rng.integers(0, 64)))
    # chain 1 of 3; its neighbours hold a state of their own that must not change
    programmes = [(1, prog)]
    oc, od = check_programme(engine, rng, 3, programmes, table, pre=[0, 1, 2] if pending else [0, 2])
    seg_chain, _, flags, _, _ = commit_seg_plan(oc, od, 3, 64)
    assert seg_chain.size == total and flags[0] & 1 and flags[-1] & 2


def test_widths_neighbouring_lanes_of_unequal_length(engine):
    """One wave whose neighbouring lanes hold segments of 0, 1, 2, 3 and 40 writes."""
    rng = np.random.default_rng(62)
    table = table_of(rng, 64)
    w = lambda k: [int(x) for x in rng.integers(0, 64, k)]
    programmes = []
    for c in range(4):  # 4 chains x 16 segments = one wave
        prog = []
        for s in range(16):
            prog += w([0, 1, 2, 3, 40][(s + c) % 5]) + ([CP] if s < 15 else [])
        if c % 2:
            prog += [CP]
        else:
            prog += w(1)
        programmes.append((c, prog))
    oc, od = check_programme(engine, rng, 4, programmes, table, pre=[1, 2])
    assert commit_seg_plan(oc, od, 4, 64)[0].size == 64


# ---- 3. empty checkpoints ---------------------------------------------------------------

def test_empty_checkpoints(engine):
    rng = np.random.default_rng(63)
    table = table_of(rng, 3)
    ch = CheckpointChains(engine, 3)
    run = lambda oc, od, tab=table: values(engine.wait(ch.submit_commit(tab, oc, od)))
    # the very first op on a fresh chain (recorder_test.go:83), and two back to back
    assert run([0, 1, 1, 1], [CP, 0, CP, CP]) == [EMPTY, hashlib.sha256(table[0].tobytes()).digest(), EMPTY]
    assert sums(ch) == [EMPTY] * 3
    # a checkpoint as the last op: the next ticket starts the chain empty
    assert run([2, 2, 2], [1, 2, CP]) == [hashlib.sha256(table[1].tobytes() + table[2].tobytes()).digest()]
    assert run([2, 2], [0, CP]) == [hashlib.sha256(table[0].tobytes()).digest()]
    assert run([2], [CP]) == [EMPTY]
    ch.write(table[:2], np.asarray([0, 1], dtype=np.uint32))
    before = sums(ch)
    # nulls only, and an empty programme: valid tickets, nothing launched, states unchanged
    t1 = ch.submit_commit(table, [0, 0, 1], [NULL, NULL, NULL])
    t2 = ch.submit_commit(table, [], [])
    t3 = ch.submit_commit(np.zeros((0, 32), np.uint8), [0, 0, 1], [NULL, CP, CP])  # an empty table
    assert t2.value == t1.value + 1 and t3.value == t2.value + 1
    assert engine.wait(t2).shape == (0, 32) and engine.wait(t1).shape == (0, 32)
    assert engine.poll(t1) and engine.poll(t2)
    assert values(engine.wait(t3)) == before[:2]
    assert sums(ch) == [EMPTY, EMPTY, before[2]]
    ch.close()


# ---- 4. equivalence with the synchronous call -------------------------------------------

def test_equivalence_with_the_synchronous_call(engine):
    rng = np.random.default_rng(64)
    n = 100
    a, b = CheckpointChains(engine, n), CheckpointChains(engine, n)
    ref = [hashlib.sha256() for _ in range(n)]
    for cycle in range(6):
        table = table_of(rng, 64)
        oc, od = random_cycle(rng, n, int(rng.integers(0, 2001)), 64)
        want = run_ref(ref, table, oc, od)
        assert values(a.commit(table, oc, od)) == want, cycle
        assert values(engine.wait(b.submit_commit(table, oc, od))) == want, cycle
        final = [r.digest() for r in ref]
        assert sums(a) == final and sums(b) == final, cycle
    a.close()
    b.close()


# ---- 5. both forms on ONE object --------------------------------------------------------

def test_both_forms_on_one_object(engine):
    """commit / write / sum / reset issued while a ticket is still in flight:
    the library orders them behind it, the caller never waits in between."""
    rng = np.random.default_rng(65)
    n = 9
    ch = CheckpointChains(engine, n)
    ref = [hashlib.sha256() for _ in range(n)]
    pending = []  # (ticket, expected values)
    for step in range(16):
        table = table_of(rng, 32)
        oc, od = random_cycle(rng, n, int(rng.integers(1, 300)), 32)
        pending.append((ch.submit_commit(table, oc, od), run_ref(ref, table, oc, od)))
        how = step % 4
        if how == 0:  # the synchronous form behind the ticket
            oc, od = random_cycle(rng, n, 60, 32)
            assert values(ch.commit(table, oc, od)) == run_ref(ref, table, oc, od), step
        elif how == 1:
            rows = table_of(rng, 5)
            to = rng.integers(0, n, 5).astype(np.uint32)
            ch.write(rows, to)
            for row, c in zip(rows, to):
                ref[int(c)].update(row.tobytes())
        elif how == 2:
            assert sums(ch) == [r.digest() for r in ref], step
        else:
            which = [int(c) for c in rng.permutation(n)[:3]]
            ch.reset(which)
            for c in which:
                ref[c] = hashlib.sha256()
    for t, want in pending:  # values of tickets retired long ago are still theirs
        assert values(engine.wait(t)) == want
    assert sums(ch) == [r.digest() for r in ref]
    ch.close()


# ---- 6. the ring ------------------------------------------------------------------------

def test_ring_six_tickets_then_the_last_and_reverse_waits(engine):
    rng = np.random.default_rng(66)
    n = 7
    ch = CheckpointChains(engine, n)
    ref = [hashlib.sha256() for _ in range(n)]
    for order in ("last_only", "reverse"):
        tickets, want = [], []
        for _ in range(6):  # more than the four slots: the fifth and sixth retire the oldest
            table = table_of(rng, 40)
            oc, od = random_cycle(rng, n, 200, 40)
            tickets.append(ch.submit_commit(table, oc, od))
            want.append(run_ref(ref, table, oc, od))
        assert [t.value for t in tickets] == list(range(tickets[0].value, tickets[0].value + 6))
        if order == "last_only":
            engine.wait(tickets[-1])  # retires every earlier ticket, in order
        else:
            for t in reversed(tickets):
                engine.wait(t)
        assert [values(t.values) for t in tickets] == want
        assert all(engine.poll(t) for t in tickets)  # retired
    table = table_of(rng, 8)
    fresh = ch.submit_commit(table, [0, 0], [3, CP])
    want = run_ref(ref, table, [0, 0], [3, CP])
    done = engine.poll(fresh)  # either answer is right for a fresh ticket
    assert isinstance(done, bool)
    assert values(engine.wait(fresh)) == want and engine.poll(fresh)
    assert sums(ch) == [r.digest() for r in ref]
    ch.close()


def test_ring_commit_tickets_between_hashing_tickets(engine):
    rng = np.random.default_rng(67)
    n = 5
    ch = CheckpointChains(engine, n)
    ref = [hashlib.sha256() for _ in range(n)]
    sha = lambda parts: hashlib.sha256(b"".join(parts)).digest()
    issued = []  # (kind, ticket, expected)
    for round_ in range(3):
        reqs = [[rng.bytes(int(k)) for k in rng.integers(0, 120, 2)] for _ in range(70)]
        issued.append(("slices", engine.submit_slices(reqs), [sha(r) for r in reqs]))
        table = table_of(rng, 48)
        oc, od = random_cycle(rng, n, 300, 48)
        issued.append(("commit", ch.submit_commit(table, oc, od), run_ref(ref, table, oc, od)))
        ln = rng.integers(0, 200, 90).astype(np.uint32)
        off = np.zeros(90, dtype=np.uint64)
        np.cumsum(ln[:-1].astype(np.uint64), out=off[1:])
        arena = rng.integers(0, 256, int(ln.sum()) + 1, dtype=np.uint8)
        issued.append(("batch", engine.submit_batch(arena, off, ln),
                       [hashlib.sha256(arena[int(o):int(o) + int(k)].tobytes()).digest() for o, k in zip(off, ln)]))
        oc, od = random_cycle(rng, n, 50, 48)
        issued.append(("commit", ch.submit_commit(table, oc, od), run_ref(ref, table, oc, od)))
        true = [sha(r) for r in reqs]
        expected = [None if i % 3 == 0 else (true[i] if i % 7 else bytes(32)) for i in range(len(reqs))]
        issued.append(("expect", engine.submit_slices_expect(reqs, expected), (true, expected)))
    assert [t.value for _, t, _ in issued] == list(range(issued[0][1].value, issued[0][1].value + len(issued)))
    for kind, t, want in reversed(issued):
        out = engine.wait(t)
        if kind == "expect":
            true, expected = want
            wrong = [i for i, e in enumerate(expected) if e is not None and e != true[i]]
            assert t.mismatches.tolist() == wrong
            for i, e in enumerate(expected):
                if e is None or i in wrong:
                    assert out[i].tobytes() == true[i]
        else:
            assert values(out) == want, kind
    assert sums(ch) == [r.digest() for r in ref]
    ch.close()


# ---- 7. where the values land -----------------------------------------------------------

@pytest.mark.parametrize("where", ["pinned_aligned", "pinned_offset_8", "pageable"])
def test_values_out_memory_kinds(engine, where):
    rng = np.random.default_rng(68)
    n = 6
    ch = CheckpointChains(engine, n)
    ref = [hashlib.sha256() for _ in range(n)]
    table = table_of(rng, 32)
    oc, od = random_cycle(rng, n, 400, 32)
    k = int(np.count_nonzero(od == CP))
    assert k > 10
    if where == "pageable":
        out = np.zeros((k, 32), dtype=np.uint8)
    else:
        raw = engine.host_empty(32 * k + 16)
        assert raw.ctypes.data % 16 == 0
        at = 8 if where == "pinned_offset_8" else 0
        out = raw[at:at + 32 * k].reshape(k, 32)
        out[:] = 0
    t = ch.submit_commit(table, oc, od, out=out)
    assert t.values is out
    assert values(engine.wait(t)) == run_ref(ref, table, oc, od)
    assert sums(ch) == [r.digest() for r in ref]
    with pytest.raises(ValueError):
        ch.submit_commit(table, oc, od, out=np.zeros((k + 1, 32), dtype=np.uint8))
    ch.close()


# ---- 8. the device form -----------------------------------------------------------------

def test_submit_commit_device_on_hashed_requests(engine):
    """Request digests written by hash_batch_device are committed where they
    lie, with no synchronisation between the two calls."""
    import torch

    rng = np.random.default_rng(69)
    n_req, n = 64, 5
    ln = rng.integers(0, 300, n_req).astype(np.uint32)
    off = np.zeros(n_req, dtype=np.uint64)
    np.cumsum(ln[:-1].astype(np.uint64), out=off[1:])
    arena = rng.integers(0, 256, int(ln.sum()) + 1, dtype=np.uint8)
    host = np.frombuffer(b"".join(hashlib.sha256(arena[int(o):int(o) + int(k)].tobytes()).digest()
                                  for o, k in zip(off, ln)), dtype=np.uint8).reshape(n_req, 32)
    d_arena = torch.from_numpy(arena).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_len = torch.from_numpy(ln.view(np.int32)).cuda()
    d_out = torch.zeros((n_req, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    oc, od = random_cycle(rng, n, 500, n_req)
    dev = CheckpointChains(engine, n)
    ref = [hashlib.sha256() for _ in range(n)]
    engine.hash_batch_device(d_arena.data_ptr(), arena.size, d_off.data_ptr(), d_len.data_ptr(), None, n_req,
                             d_out.data_ptr())
    t = dev.submit_commit_device(d_out.data_ptr(), n_req, oc, od, keep=d_out)  # behind the hashing, no sync
    want = run_ref(ref, host, oc, od)
    assert values(engine.wait(t)) == want and len(want) > 10
    assert sums(dev) == [r.digest() for r in ref]
    engine.sync()
    assert np.array_equal(d_out.cpu().numpy(), host)
    with pytest.raises(MirshaError, match="16-byte aligned"):
        dev.submit_commit_device(d_out.data_ptr() + 4, n_req - 1, oc[:1], od[:1] * 0)
    dev.close()


# ---- 9. validation failures -------------------------------------------------------------

def test_validation_failures_queue_nothing(engine):
    rng = np.random.default_rng(70)
    n = 6
    ch = CheckpointChains(engine, n)
    table = table_of(rng, 8)
    ch.write(table[:5], np.asarray([0, 1, 1, 3, 5], dtype=np.uint32))
    before = sums(ch)
    t0 = ch.submit_commit(table, [], [])  # an empty programme: a ticket all the same
    with pytest.raises(MirshaError, match=r"op_chain\[1\] = 6 >= 6"):
        ch.submit_commit(table, [0, 6], [0, 1])
    with pytest.raises(MirshaError, match=r"op_digest\[2\] = 8 >= 8"):
        ch.submit_commit(table, [0, 1, 2], [0, 1, 8])
    # checkpoints without values_out: the raw call (the Python layer always passes one)
    oc = np.asarray([0, 1, 2], dtype=np.uint32)
    od = np.asarray([0, CP, 1], dtype=np.uint32)
    k, t = ctypes.c_uint32(77), ctypes.c_uint64(77)
    with pytest.raises(MirshaError, match="NULL values_out"):
        engine._check(engine._lib.mirsha_chains_commit_submit(engine.ctx, ch.handle, table.ctypes.data, 8,
                                                              oc.ctypes.data, od.ctypes.data, 3, None,
                                                              ctypes.byref(k), ctypes.byref(t)))
    assert t.value == 77  # no ticket was handed out
    assert sums(ch) == before
    t1 = ch.submit_commit(table, oc, od)
    assert t1.value == t0.value + 1  # the failures consumed no ticket
    ref1 = hashlib.sha256(table[1].tobytes() + table[2].tobytes())
    assert values(engine.wait(t1)) == [ref1.digest()]
    assert engine.poll(t0)
    ch.close()


# ---- 10. Processor / ProcessorWorkPool --------------------------------------------------

class NodeState:
    """testengine's application state restated (recorder.go:186-256)."""

    def __init__(self):
        self.active = hashlib.sha256()

    def commit(self, commits):
        out = []
        for c in commits:
            if c.batch is not None:
                for d in c.batch.digests:
                    self.active.update(d or b"")
            else:
                out.append(self.active.digest())
                self.active = hashlib.sha256()
        return out


def sha(parts):
    return hashlib.sha256(b"".join(parts)).digest()


def six_cycles(seed):
    """Hashes with and without expectations (two of them wrong), a cycle
    without commits, a cycle with only commits."""
    rng = np.random.default_rng(seed)
    cycles, seq = [], 0
    for cycle in range(6):
        reqs = []
        for i in range(0 if cycle == 4 else 25):
            data = [rng.bytes(int(k)) for k in rng.integers(0, 90, 3)]
            expected = None if i % 3 == 0 or cycle == 1 else (sha(data) if i % 11 else bytes(32))
            reqs.append(HashRequest(data=data, origin=(cycle, i), expected=expected))
        commits = []
        for _ in range(0 if cycle == 2 else 7):
            seq += 1
            digests = [None if rng.random() < 0.15 else rng.bytes(32) for _ in range(int(rng.integers(0, 6)))]
            commits.append(Commit(batch=CommitBatch(digests, seq_no=seq)))
            if seq % 3 == 0:  # a checkpoint in the middle of the list
                commits.append(Commit(checkpoint=Checkpoint(seq_no=seq)))
        cycles.append((reqs, commits))
    return cycles


def check_cycle(res, reqs, commits, want_values):
    assert [r.digest for r in res.digests] == [sha(q.data) for q in reqs]
    assert all(r.request is q for r, q in zip(res.digests, reqs))
    asked = [c for c in commits if c.checkpoint is not None]
    assert [r.value for r in res.checkpoints] == want_values
    assert [r.commit for r in res.checkpoints] == asked
    assert all(r.checkpoint is c.checkpoint for r, c in zip(res.checkpoints, asked))


@pytest.mark.parametrize("cls", [Processor, ProcessorWorkPool])
@pytest.mark.parametrize("verify", [False, True], ids=["plain", "verify_on_device"])
def test_processor_async_commits_on_and_off(engine, cls, verify):
    cycles = six_cycles(71)
    state = NodeState()
    want = [state.commit(c) for _, c in cycles]
    assert sum(map(len, want)) >= 8
    results = {}
    for flag in (False, True):
        log = DeviceLog(engine)
        p = cls(engine=engine, log=log, verify_on_device=verify, async_commits=flag)
        pend = [p.submit(Actions(hash=r, commits=c)) for r, c in cycles]
        got = [None] * len(cycles)
        for k in reversed(range(len(cycles))):  # cycles committed in submission order all the same
            got[k] = pend[k].wait()
        for res, (reqs, commits), w in zip(got, cycles, want):
            check_cycle(res, reqs, commits, w)
        assert log.chains.sum([0])[0].tobytes() == state.active.digest()
        results[flag] = [([r.digest for r in res.digests], [r.value for r in res.checkpoints]) for res in got]
        log.close()
    assert results[True] == results[False]


def test_work_pool_process_with_async_commits(engine):
    cycles = six_cycles(72)
    state = NodeState()
    log = DeviceLog(engine)
    pool = ProcessorWorkPool(engine=engine, log=log, async_commits=True)
    ran = []
    for reqs, commits in cycles:
        res = pool.process(Actions(hash=reqs, commits=commits), overlap=lambda: ran.append(1))
        check_cycle(res, reqs, commits, state.commit(commits))
    assert len(ran) == 6
    plain = Processor(engine=engine, log=log, async_commits=True)  # process() is the synchronous path
    reqs, commits = cycles[0]
    check_cycle(plain.process(Actions(hash=reqs, commits=commits)), reqs, commits, state.commit(commits))
    assert log.chains.sum([0])[0].tobytes() == state.active.digest()
    log.close()


# ---- 11. the four-node log --------------------------------------------------------------

def test_testengine_log_of_four_nodes_on_golden_digests(engine, layouts):
    """The golden checkpoint chain (60 testengine requests committed in
    batches of 5, checkpoints after 20, 40 and 60 and one more on the empty
    state) through a 4-node DeviceLog with async_commits: one ticket per
    cycle, the table passed once for the four nodes."""
    digest = {(r["client"], r["req_no"]): bytes.fromhex(r["sha256"]) for r in layouts["testengine_requests"]}
    cc = layouts["checkpoint_chain"]
    order = [digest[(c, r)] for c, r in cc["commits"]]
    commits, start = [], 0
    for cp in cc["checkpoints"]:
        for lo in range(start, cp["after_commit"], 5):
            commits.append(Commit(batch=CommitBatch(order[lo:lo + 5], seq_no=lo // 5 + 1)))
        start = cp["after_commit"]
        commits.append(Commit(checkpoint=Checkpoint(seq_no=start // 5)))
    want = [bytes.fromhex(cp.get("sha256") or cp.get("empty_after_reset")) for cp in cc["checkpoints"]]
    log = DeviceLog(engine, n_nodes=4, node=2)
    p = Processor(engine=engine, log=log, async_commits=True)
    reqs = [HashRequest(data=hashdata.request_hash_data(r["client"], r["req_no"],
                                                        hashdata.testengine_request_payload(r["client"], r["req_no"])))
            for r in layouts["testengine_requests"][:40]]
    cut = 9  # two cycles: the cut falls between a batch and its checkpoint
    pend = [p.submit(Actions(hash=reqs, commits=part)) for part in (commits[:cut], commits[cut:])]
    got = []
    for pending in pend:
        res = pending.wait()
        assert [r.digest.hex() for r in res.digests] == [r["sha256"] for r in layouts["testengine_requests"][:40]]
        got += [r.value for r in res.checkpoints]
        assert log.values.shape == (len(res.checkpoints), 4, 32)
        for node in range(4):  # every node's chain holds the same value
            assert [v.tobytes() for v in log.values[:, node]] == [r.value for r in res.checkpoints]
    assert got == want
    assert sums(log.chains) == [EMPTY] * 4
    log.close()


# ---- 12. the C++ host mirror ------------------------------------------------------------

@pytest.mark.parametrize("flags", [4, 6], ids=["process_with_option", "submit_wait_async_commits"])
def test_cpp_host_mirror_async_commits(flags):
    """mirbft::Processor(async_commits) with a 3-node mirbft::DeviceLog
    (mirbft_amd/host): bit 2 of mirbft_host_commit's flags selects the option;
    the C entry itself checks the order and the back-pointers."""
    rng = np.random.default_rng(73)
    host = ctypes.CDLL(_lib.HOST_LIB_PATH)
    assert host.mirbft_host_features() & 1  # this build knows the flag (an older one would ignore it)
    batch_len = [3, 0, 0xFFFFFFFF, 0xFFFFFFFF, 5, 1, 0xFFFFFFFF, 2]
    rows = [None if k in (1, 6) else rng.bytes(32) for k in range(11)]
    bufs = [ctypes.create_string_buffer(r, 32) if r is not None else None for r in rows]
    ptrs = (ctypes.c_void_p * len(rows))(*[ctypes.addressof(b) if b is not None else None for b in bufs])
    lens = (ctypes.c_uint32 * len(batch_len))(*batch_len)
    n_nodes = 3
    out = (ctypes.c_uint8 * (32 * 3 * n_nodes))()
    k = ctypes.c_uint32(0)
    err = ctypes.create_string_buffer(256)
    host.mirbft_host_commit.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                        ctypes.c_char_p, ctypes.c_uint32]
    rc = host.mirbft_host_commit(0, n_nodes, ptrs, lens, len(batch_len), out, ctypes.byref(k), flags, err, 256)
    assert rc == 0, err.value
    state, want, at = hashlib.sha256(), [], 0
    for m in batch_len:
        if m == 0xFFFFFFFF:
            want.append(state.digest())
            state = hashlib.sha256()
        else:
            for r in rows[at:at + m]:
                state.update(r or b"")
            at += m
    assert k.value == 3 and want[1] == EMPTY
    got = [bytes(out[32 * i:32 * i + 32]) for i in range(3 * n_nodes)]
    assert got == [w for w in want for _ in range(n_nodes)]
