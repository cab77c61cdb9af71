"""Host side of the commits' ring form, no GPU: mirsha_commit_seg_plan (the
arrays mirsha_chains_commit_submit sends to the device) through ctypes against
a short Python restatement and against hashlib (each segment hashed on its
own gives the values and the leftover hashers of the sequential walk), and the
``async_commits`` plumbing of Processor / ProcessorWorkPool over a fake engine
and a fake log."""
import ctypes
import hashlib

import numpy as np
import pytest

from mirbft_amd import (ActionResults, Actions, Checkpoint, Commit, CommitBatch, HashRequest, MirshaError, Processor,
                        ProcessorWorkPool, _lib, commit_plan, commit_seg_plan)

NULL = _lib.MIRSHA_NULL_INDEX
CP = _lib.MIRSHA_COMMIT_CHECKPOINT
FLAG = _lib.MIRSHA_COMMIT_ENTRY_CHECKPOINT
FIRST = _lib.MIRSHA_COMMIT_SEG_FIRST
LAST = _lib.MIRSHA_COMMIT_SEG_LAST
GUARD = 0xDEADBEEF


# ---- mirsha_commit_seg_plan --------------------------------------------------------

def seg_raw(op_chain, op_digest, n_chains, n_digests, n_ops=None, null_chain=False, null_digest=False):
    """The C call with guard words behind every output; returns
    (rc, seg_chain, sfirst, seg_flags, ent, (n_active, n_values), bad_op)."""
    oc = np.ascontiguousarray(op_chain, dtype=np.uint32)
    od = np.ascontiguousarray(op_digest, dtype=np.uint32)
    n = oc.size if n_ops is None else n_ops
    seg_chain = np.full(n + 1, GUARD, dtype=np.uint32)
    sfirst = np.full(n + 2, GUARD, dtype=np.uint32)
    seg_flags = np.full(n + 1, GUARD, dtype=np.uint32)
    ent = np.full(n + 1, GUARD, dtype=np.uint32)
    ns, na, ne, nv, bad = (ctypes.c_uint32(GUARD) for _ in range(5))
    rc = _lib.load().mirsha_commit_seg_plan(None if null_chain or not oc.size else oc.ctypes.data,
                                            None if null_digest or not od.size else od.ctypes.data, n, n_chains,
                                            n_digests, seg_chain.ctypes.data, sfirst.ctypes.data,
                                            seg_flags.ctypes.data, ent.ctypes.data, ctypes.byref(ns), ctypes.byref(na),
                                            ctypes.byref(ne), ctypes.byref(nv), ctypes.byref(bad))
    if rc == _lib.MIRSHA_OK:
        k = ns.value
        assert seg_chain[k] == GUARD and seg_flags[k] == GUARD and ent[ne.value] == GUARD
        assert sfirst[k + 1] == GUARD or (n == 0 and k == 0)
        assert bad.value == 0xFFFFFFFF
        return rc, seg_chain[:k], sfirst[:k + 1], seg_flags[:k], ent[:ne.value], (na.value, nv.value), None
    assert ns.value == 0
    return rc, None, None, None, None, None, bad.value


def seg_python(op_chain, op_digest):
    """The restatement: per chain its ops in op order, nulls dropped,
    checkpoints numbered in op order across all chains; each chain's list cut
    after every checkpoint, no empty piece behind a final checkpoint."""
    per, rows = {}, 0
    for c, d in zip(op_chain, op_digest):
        c, d = int(c), int(d)
        if d == NULL:
            continue
        if d == CP:
            per.setdefault(c, []).append(FLAG | rows)
            rows += 1
        else:
            per.setdefault(c, []).append(d)
    seg_chain, sfirst, flags, ent = [], [0], [], []
    for c in sorted(per):
        pieces, cur = [], []
        for x in per[c]:
            cur.append(x)
            if x & FLAG:
                pieces.append(cur)
                cur = []
        if cur:
            pieces.append(cur)
        for k, piece in enumerate(pieces):
            seg_chain.append(c)
            flags.append((FIRST if k == 0 else 0) | (LAST if k == len(pieces) - 1 else 0))
            ent += piece
            sfirst.append(len(ent))
    return seg_chain, sfirst, flags, ent, (len(per), rows)


def check_plan(oc, od, n_chains, n_digests):
    rc, seg_chain, sfirst, flags, ent, counts, _ = seg_raw(oc, od, n_chains, n_digests)
    assert rc == _lib.MIRSHA_OK
    want = seg_python(oc, od)
    assert (seg_chain.tolist(), sfirst.tolist(), flags.tolist(), ent.tolist(), counts) == want
    # ent[] and the counts are mirsha_commit_plan's, unchanged
    act, efirst, p_ent, nv = commit_plan(oc, od, n_chains, n_digests)
    assert p_ent.tolist() == ent.tolist() and nv == counts[1] and act.size == counts[0]
    # n_seg = active chains + checkpoint entries that are not their chain's final entry
    final = set(int(e) - 1 for e in efirst[1:])
    inner = sum(1 for e, x in enumerate(ent.tolist()) if x & FLAG and e not in final)
    assert seg_chain.size == act.size + inner
    # the Python helper returns the same arrays
    h = commit_seg_plan(oc, od, n_chains, n_digests)
    assert (h[0].tolist(), h[1].tolist(), h[2].tolist(), h[3].tolist(), h[4]) == want[:4] + (counts[1],)
    return seg_chain, sfirst, flags, ent


def parity_classes():
    """tests/test_gpu_commits.py's: (entry parity, writes before the first
    checkpoint, writes between two checkpoints or None for a single
    checkpoint, writes after the last)."""
    return [(odd, a, m, b) for odd in (0, 1) for a in range(4) for m in (None, 0, 1, 2, 3) for b in range(4)]


def class_programmes(rng, n_digests=16):
    progs = []
    for _, a, m, b in parity_classes():
        w = lambda k: [int(x) for x in rng.integers(0, n_digests, k)]
        progs.append(w(a) + [CP] + ([] if m is None else w(m) + [CP]) + w(b))
    return progs


def interleave(rng, programmes):
    owner = np.concatenate([np.full(len(p), k, dtype=np.int64) for k, p in enumerate(programmes)])
    rng.shuffle(owner)
    at = [0] * len(programmes)
    oc, od = [], []
    for k in owner:
        oc.append(int(k))
        od.append(programmes[k][at[k]])
        at[k] += 1
    return np.asarray(oc, dtype=np.uint32), np.asarray(od, dtype=np.uint32)


def walk_segments(table, state, seg_chain, sfirst, flags, ent, n_values):
    """The plan's algebra on hashlib: every segment on a hasher of its own (a
    FIRST one continues the chain's), a LAST one's hasher becomes the chain's.
    ``state[c]`` = the chain's hashlib object; returns the values by row."""
    out = [None] * n_values
    for s in range(len(seg_chain)):
        c = int(seg_chain[s])
        h = state[c].copy() if flags[s] & FIRST else hashlib.sha256()
        for x in ent[int(sfirst[s]):int(sfirst[s + 1])]:
            x = int(x)
            if x & FLAG:
                out[x & ~FLAG] = h.digest()
                h = hashlib.sha256()
            else:
                h.update(table[x].tobytes())
        if flags[s] & LAST:
            state[c] = h
    return out


def walk_sequential(table, state, oc, od):
    out = []
    for c, d in zip(oc, od):
        c, d = int(c), int(d)
        if d == NULL:
            continue
        if d == CP:
            out.append(state[c].digest())
            state[c] = hashlib.sha256()
        else:
            state[c].update(table[d].tobytes())
    return out


def check_algebra(rng, oc, od, n_chains, n_digests, plan):
    table = rng.integers(0, 256, (max(n_digests, 1), 32), dtype=np.uint8)
    seq = [hashlib.sha256(b"x" * (32 * (c % 3))) for c in range(n_chains)]  # any entry parity
    seg = [h.copy() for h in seq]
    want = walk_sequential(table, seq, oc, od)
    got = walk_segments(table, seg, *plan, len(want))
    assert got == want
    assert [h.digest() for h in seg] == [h.digest() for h in seq]


def test_seg_plan_parity_classes():
    rng = np.random.default_rng(41)
    progs = class_programmes(rng)
    oc, od = interleave(rng, progs)
    plan = check_plan(oc, od, len(progs), 16)
    check_algebra(rng, oc, od, len(progs), 16, plan)
    for c, prog in enumerate(progs):  # each class as a programme of its own
        oc1 = np.full(len(prog), c, dtype=np.uint32)
        plan = check_plan(oc1, np.asarray(prog, dtype=np.uint32), len(progs), 16)
        cps = prog.count(CP)
        assert len(plan[0]) == cps + (prog[-1] != CP)
        check_algebra(rng, oc1, prog, len(progs), 16, plan)


def random_programme(rng, n_chains, n_ops, n_digests, p_null, p_cp):
    named = rng.permutation(n_chains)[:max(1, n_chains - n_chains // 3)]  # some chains never named
    oc = rng.choice(named, n_ops).astype(np.uint32)
    kind = rng.random(n_ops)
    od = rng.integers(0, max(n_digests, 1), n_ops).astype(np.uint32)
    od[kind < p_null] = NULL
    od[kind > 1.0 - p_cp] = CP
    if n_digests == 0:
        od[(od != NULL) & (od != CP)] = NULL
    return oc, od


def test_seg_plan_random_programmes():
    for seed in range(200):
        rng = np.random.default_rng(5000 + seed)
        n_chains = int(rng.integers(1, 120))
        n_ops = int(rng.integers(0, 600)) if seed else 0
        n_digests = int(rng.integers(0, 64))
        oc, od = random_programme(rng, n_chains, n_ops, n_digests, rng.random() * 0.4, rng.random() * 0.5)
        plan = check_plan(oc, od, n_chains, n_digests)
        check_algebra(rng, oc, od, n_chains, n_digests, plan)


def test_seg_plan_flags_and_final_checkpoint():
    # chain 0: w CP w -> two segments; chain 1: w w CP -> ONE segment (no empty one behind it);
    # chain 2: CP CP -> two segments of one checkpoint; chain 3: only nulls -> not active
    oc = np.asarray([0, 1, 2, 0, 1, 3, 2, 0, 1], dtype=np.uint32)
    od = np.asarray([5, 6, CP, CP, 7, NULL, CP, 4, CP], dtype=np.uint32)
    rc, seg_chain, sfirst, flags, ent, counts, _ = seg_raw(oc, od, 4, 8)
    assert rc == _lib.MIRSHA_OK and counts == (3, 4)
    assert seg_chain.tolist() == [0, 0, 1, 2, 2]
    assert sfirst.tolist() == [0, 2, 3, 6, 7, 8]
    assert flags.tolist() == [FIRST, LAST, FIRST | LAST, FIRST, LAST]
    assert ent.tolist() == [5, FLAG | 1, 4, 6, 7, FLAG | 3, FLAG | 0, FLAG | 2]


def test_seg_plan_empty_and_nulls_only():
    rc, seg_chain, sfirst, flags, ent, counts, _ = seg_raw([], [], 4, 9)
    assert rc == _lib.MIRSHA_OK and seg_chain.size == 0 and ent.size == 0 and counts == (0, 0)
    rc, seg_chain, sfirst, flags, ent, counts, _ = seg_raw([0, 3, 3], [NULL] * 3, 4, 0)
    assert rc == _lib.MIRSHA_OK and seg_chain.size == 0 and sfirst.tolist() == [0] and counts == (0, 0)
    assert commit_seg_plan([], [], 4, 9)[4] == 0


@pytest.mark.parametrize("oc, od, n_chains, n_digests, bad", [
    ([0, 4, 1], [0, 1, 2], 4, 3, 1),           # chain id == n_chains
    ([0, 1, 2 ** 32 - 1], [0, 1, CP], 4, 3, 2),  # chain id far out, on a checkpoint op
    ([0, 1, 2], [0, 3, 1], 4, 3, 1),           # digest index == n_digests
    ([0, 1, 2], [0, 1, CP - 1], 4, 3, 2),      # just below the markers
    ([0], [0], 4, 0, 0),                       # a write into an empty table
    ([0, 9], [NULL, NULL], 4, 0, 1),           # a null write still names a chain
    ([0], [CP], 0, 0, 0),                      # no chains at all
])
def test_seg_plan_rejects_and_names_the_op(oc, od, n_chains, n_digests, bad):
    """The error cases of commit_plan (tests/test_commit_host.py)."""
    rc, *_, bad_op = seg_raw(oc, od, n_chains, n_digests)
    assert rc == _lib.MIRSHA_EINVAL and bad_op == bad
    with pytest.raises(MirshaError, match=f"op {bad}"):
        commit_seg_plan(oc, od, n_chains, n_digests)


def test_seg_plan_null_arrays_and_limits():
    assert seg_raw([0, 1], [0, 1], 4, 3, null_chain=True)[0] == _lib.MIRSHA_EINVAL
    assert seg_raw([0, 1], [0, 1], 4, 3, null_digest=True)[0] == _lib.MIRSHA_EINVAL
    lib = _lib.load()
    oc = np.zeros(2, dtype=np.uint32)
    out = np.zeros(8, dtype=np.uint32)
    p = out.ctypes.data
    cnt = ctypes.c_uint32(0)
    args = (oc.ctypes.data, oc.ctypes.data, 2, 4, 3)
    for k in range(4):  # a NULL output array with ops to plan
        arrays = [p] * 4
        arrays[k] = None
        assert lib.mirsha_commit_seg_plan(*args, *arrays, cnt, cnt, cnt, cnt, None) == _lib.MIRSHA_EINVAL
    for k in range(4):  # NULL count outputs
        counts = [cnt] * 4
        counts[k] = None
        assert lib.mirsha_commit_seg_plan(*args, p, p, p, p, *counts, None) == _lib.MIRSHA_EINVAL
    # an entry's low 31 bits hold the digest index or the row
    assert seg_raw([0], [0], 4, FLAG + 1)[0] == _lib.MIRSHA_ERANGE
    assert seg_raw([0], [FLAG - 1], 4, FLAG)[0] == _lib.MIRSHA_OK


def test_signatures_hold_the_new_entry_points():
    sig = _lib.SIGNATURES
    base = sig["mirsha_chains_commit"]
    for name in ("mirsha_chains_commit_submit", "mirsha_chains_commit_submit_device"):
        restype, args = sig[name]
        assert restype is ctypes.c_int and args[:-1] == base[1] and args[-1] is ctypes.POINTER(ctypes.c_uint64)
    restype, args = sig["mirsha_commit_seg_plan"]
    assert restype is ctypes.c_int and len(args) == 14
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in ("mirsha_commit_seg_plan", "mirsha_chains_commit_submit",
                                         "mirsha_chains_commit_submit_device"))


# ---- async_commits plumbing ------------------------------------------------------------

def sha(parts):
    return hashlib.sha256(b"".join(parts)).digest()


def d32(k):
    return hashlib.sha256(b"req%d" % k).digest()


class FakeTicket:
    def __init__(self, out):
        self.out = out


class FakeEngine:
    def __init__(self):
        self.calls = []

    def hash_slices(self, requests, dedup=False):
        self.calls.append("hash_slices")
        return np.frombuffer(b"".join(sha(r) for r in requests), dtype=np.uint8).reshape(len(requests), 32)

    def submit_slices(self, requests, dedup=False):
        self.calls.append("submit_slices")
        return FakeTicket(np.frombuffer(b"".join(sha(r) for r in requests), dtype=np.uint8).reshape(len(requests), 32))

    def wait(self, ticket):
        self.calls.append("wait")
        return ticket.out

    def poll(self, ticket):
        return True


class SyncLog:
    """NodeState restated (recorder.go:186-256); only the synchronous call."""

    def __init__(self, calls):
        self.h = hashlib.sha256()
        self.calls = calls

    def apply(self, commits):
        out = []
        for c in commits:
            if c.batch is not None:
                for d in c.batch.digests:
                    self.h.update(d or b"")
            else:
                out.append(self.h.digest())
                self.h = hashlib.sha256()
        return out

    def commit_cycle(self, commits):
        self.calls.append("commit_cycle")
        return self.apply(commits)


class AsyncLog(SyncLog):
    """The same with the asynchronous pair: applied in submission order."""

    def submit_cycle(self, commits):
        self.calls.append("submit_cycle")
        return FakeTicket(self.apply(commits))

    def collect_cycle(self, ticket):
        self.calls.append("collect_cycle")
        return ticket.out


def cycle(k=0):
    reqs = [HashRequest(data=[b"a", b"bc%d" % k], origin=1), HashRequest(data=[b""], origin=2)]
    commits = [Commit(batch=CommitBatch([d32(k), d32(1)], seq_no=1)), Commit(checkpoint=Checkpoint(seq_no=1)),
               Commit(checkpoint=Checkpoint(seq_no=1)), Commit(batch=CommitBatch([None, d32(2)], seq_no=2)),
               Commit(checkpoint=Checkpoint(seq_no=2)), Commit(batch=CommitBatch([d32(3)], seq_no=3))]
    return reqs, commits


def check_results(res, reqs, commits, want):
    assert isinstance(res, ActionResults)
    assert [r.digest for r in res.digests] == [sha(q.data) for q in reqs]
    assert all(r.request is q for r, q in zip(res.digests, reqs))
    asked = [c for c in commits if c.checkpoint is not None]
    assert [r.value for r in res.checkpoints] == want
    assert all(r.commit is c and r.checkpoint is c.checkpoint for r, c in zip(res.checkpoints, asked))


@pytest.mark.parametrize("cls", [Processor, ProcessorWorkPool])
def test_async_commits_queue_first_and_collect_at_wait(cls):
    eng = FakeEngine()
    log = AsyncLog(eng.calls)
    p = cls(engine=eng, log=log, async_commits=True)
    ref = SyncLog([])
    cycles = [cycle(k) for k in range(3)]
    pend = [p.submit(Actions(hash=r, commits=c)) for r, c in cycles]
    # the commits are queued ahead of the hashing, cycle by cycle, and nothing is collected yet
    assert eng.calls == ["submit_cycle", "submit_slices"] * 3
    want = [ref.apply(c) for _, c in cycles]
    for k in (2, 0, 1):  # waits in any order: cycles were committed in submission order
        res = pend[k].wait()
        check_results(res, *cycles[k], want[k])
        assert pend[k].wait() is res
    assert eng.calls.count("collect_cycle") == 3 and "commit_cycle" not in eng.calls
    assert pend[0].done()


def test_async_commits_off_is_todays_sequence():
    eng = FakeEngine()
    log = AsyncLog(eng.calls)
    reqs, commits = cycle()
    res = Processor(engine=eng, log=log).submit(Actions(hash=reqs, commits=commits)).wait()
    assert eng.calls == ["commit_cycle", "submit_slices", "wait"]
    check_results(res, reqs, commits, SyncLog([]).apply(commits))


def test_async_commits_with_a_log_without_submit_cycle_falls_to_the_synchronous_call():
    eng = FakeEngine()
    log = SyncLog(eng.calls)
    reqs, commits = cycle()
    res = Processor(engine=eng, log=log, async_commits=True).submit(Actions(hash=reqs, commits=commits)).wait()
    assert eng.calls == ["commit_cycle", "submit_slices", "wait"]
    check_results(res, reqs, commits, SyncLog([]).apply(commits))


def test_async_commits_process_is_unchanged_and_pool_has_the_reference_shape():
    eng = FakeEngine()
    log = AsyncLog(eng.calls)
    reqs, commits = cycle()
    want = SyncLog([]).apply(commits)
    res = Processor(engine=eng, log=log, async_commits=True).process(Actions(hash=reqs, commits=commits))
    assert eng.calls == ["hash_slices", "commit_cycle"]  # process(): the hash loop, then the commit loop
    check_results(res, reqs, commits, want)
    del eng.calls[:]
    log.h = hashlib.sha256()
    pool = ProcessorWorkPool(engine=eng, log=log, async_commits=True)
    res = pool.process(Actions(hash=reqs, commits=commits), overlap=lambda: eng.calls.append("overlap"))
    assert eng.calls == ["submit_cycle", "submit_slices", "overlap", "collect_cycle", "wait"]
    check_results(res, reqs, commits, want)


def test_async_commits_edge_cycles():
    eng = FakeEngine()
    log = AsyncLog(eng.calls)
    p = Processor(engine=eng, log=log, async_commits=True)
    reqs, commits = cycle()
    res = p.submit(Actions(hash=reqs)).wait()  # no commits: the log is not called
    assert res.checkpoints == [] and "submit_cycle" not in eng.calls
    res = p.submit(Actions(commits=commits)).wait()  # only commits
    assert res.digests == [] and [r.value for r in res.checkpoints] == SyncLog([]).apply(commits)
    with pytest.raises(RuntimeError, match="log"):
        Processor(engine=eng, async_commits=True).submit(Actions(commits=commits))

    class Short(AsyncLog):
        def collect_cycle(self, ticket):
            return ticket.out[:-1]

    with pytest.raises(RuntimeError, match="2 values for 3 checkpoints"):
        Processor(engine=eng, log=Short([]), async_commits=True).submit(Actions(commits=commits)).wait()
