"""Host side of the commit path, no GPU: mirsha_commit_plan (the arrays
mirsha_chains_commit sends to the device) through ctypes against a short
Python restatement, and the Actions / Commit / CheckpointResult plumbing of
Processor.process / submit / ProcessorWorkPool.process over a fake engine and
a fake log."""
import ctypes
import hashlib

import numpy as np
import pytest

from mirbft_amd import (ActionResults, Actions, Checkpoint, CheckpointResult, Commit, CommitBatch, HashRequest,
                        MirshaError, Processor, ProcessorWorkPool, _lib, commit_plan, commit_programme)

NULL = _lib.MIRSHA_NULL_INDEX
CP = _lib.MIRSHA_COMMIT_CHECKPOINT
FLAG = _lib.MIRSHA_COMMIT_ENTRY_CHECKPOINT
GUARD = 0xDEADBEEF


# ---- mirsha_commit_plan -----------------------------------------------------------

def plan_raw(op_chain, op_digest, n_chains, n_digests, n_ops=None, null_chain=False, null_digest=False):
    """The C call with guard words behind every output; returns
    (rc, act, efirst, ent, n_values, bad_op)."""
    oc = np.ascontiguousarray(op_chain, dtype=np.uint32)
    od = np.ascontiguousarray(op_digest, dtype=np.uint32)
    n = oc.size if n_ops is None else n_ops
    cap = min(n, n_chains)
    act = np.full(cap + 1, GUARD, dtype=np.uint32)
    efirst = np.full(cap + 2, GUARD, dtype=np.uint32)
    ent = np.full(n + 1, GUARD, dtype=np.uint32)
    na, ne, nv, bad = (ctypes.c_uint32(GUARD) for _ in range(4))
    rc = _lib.load().mirsha_commit_plan(None if null_chain or not oc.size else oc.ctypes.data,
                                        None if null_digest or not od.size else od.ctypes.data, n, n_chains,
                                        n_digests, act.ctypes.data, efirst.ctypes.data, ent.ctypes.data,
                                        ctypes.byref(na), ctypes.byref(ne), ctypes.byref(nv), ctypes.byref(bad))
    if rc == _lib.MIRSHA_OK:
        assert act[na.value] == GUARD and efirst[na.value + 1] == GUARD and ent[ne.value] == GUARD
        assert bad.value == 0xFFFFFFFF
        return rc, act[:na.value], efirst[:na.value + 1], ent[:ne.value], nv.value, None
    return rc, None, None, None, None, bad.value


def plan_python(op_chain, op_digest, n_chains):
    """The restatement: per chain its ops in op order, nulls dropped,
    checkpoints numbered in op order across all chains."""
    per = {}
    rows = 0
    for c, d in zip(op_chain, op_digest):
        c, d = int(c), int(d)
        if d == NULL:
            continue
        if d == CP:
            per.setdefault(c, []).append(FLAG | rows)
            rows += 1
        else:
            per.setdefault(c, []).append(d)
    act = sorted(per)
    efirst, ent = [0], []
    for c in act:
        ent += per[c]
        efirst.append(len(ent))
    return act, efirst, ent, rows


def random_programme(rng, n_chains, n_ops, n_digests, p_null=0.15, p_cp=0.1):
    named = rng.permutation(n_chains)[:max(1, n_chains - n_chains // 3)]  # some chains never named
    oc = rng.choice(named, n_ops).astype(np.uint32)
    kind = rng.random(n_ops)
    od = rng.integers(0, max(n_digests, 1), n_ops).astype(np.uint32)
    od[kind < p_null] = NULL
    od[kind > 1.0 - p_cp] = CP
    if n_digests == 0:
        od[(od != NULL) & (od != CP)] = NULL
    return oc, od


@pytest.mark.parametrize("seed", range(24))
def test_commit_plan_matches_restatement(seed):
    rng = np.random.default_rng(1000 + seed)
    n_chains = int(rng.integers(1, 301))
    n_ops = int(rng.integers(0, 2001)) if seed else 0
    n_digests = int(rng.integers(0, 500))
    oc, od = random_programme(rng, n_chains, n_ops, n_digests, p_null=rng.random() * 0.4, p_cp=rng.random() * 0.4)
    rc, act, efirst, ent, nv, _ = plan_raw(oc, od, n_chains, n_digests)
    assert rc == _lib.MIRSHA_OK
    want = plan_python(oc, od, n_chains)
    assert (act.tolist(), efirst.tolist(), ent.tolist(), nv) == want
    # the Python helper returns the same arrays
    h_act, h_first, h_ent, h_nv = commit_plan(oc, od, n_chains, n_digests)
    assert (h_act.tolist(), h_first.tolist(), h_ent.tolist(), h_nv) == want


def test_commit_plan_only_checkpoints_rows_in_op_order():
    oc = np.asarray([5, 0, 5, 2, 0, 5], dtype=np.uint32)
    od = np.full(6, CP, dtype=np.uint32)
    rc, act, efirst, ent, nv, _ = plan_raw(oc, od, 8, 0)
    assert rc == _lib.MIRSHA_OK and nv == 6
    assert act.tolist() == [0, 2, 5] and efirst.tolist() == [0, 2, 3, 6]
    # chain 0 has ops 1 and 4, chain 2 op 3, chain 5 ops 0, 2, 5: the row is the op's rank
    assert ent.tolist() == [FLAG | 1, FLAG | 4, FLAG | 3, FLAG | 0, FLAG | 2, FLAG | 5]


def test_commit_plan_rows_count_checkpoints_only():
    oc = np.asarray([1, 1, 0, 1, 0, 0], dtype=np.uint32)
    od = np.asarray([7, CP, 3, NULL, CP, 2], dtype=np.uint32)
    rc, act, efirst, ent, nv, _ = plan_raw(oc, od, 2, 8)
    assert rc == _lib.MIRSHA_OK and nv == 2
    assert act.tolist() == [0, 1] and efirst.tolist() == [0, 3, 5]
    assert ent.tolist() == [3, FLAG | 1, 2, 7, FLAG | 0]


def test_commit_plan_only_nulls_has_no_active_chain():
    oc = np.asarray([0, 3, 3, 1], dtype=np.uint32)
    od = np.full(4, NULL, dtype=np.uint32)
    rc, act, efirst, ent, nv, _ = plan_raw(oc, od, 4, 0)
    assert rc == _lib.MIRSHA_OK
    assert act.size == 0 and efirst.tolist() == [0] and ent.size == 0 and nv == 0


def test_commit_plan_empty():
    rc, act, efirst, ent, nv, _ = plan_raw([], [], 4, 9)
    assert rc == _lib.MIRSHA_OK and act.size == 0 and efirst.tolist() == [0] and ent.size == 0 and nv == 0
    assert commit_plan([], [], 4, 9)[3] == 0


@pytest.mark.parametrize("oc, od, n_chains, n_digests, bad", [
    ([0, 4, 1], [0, 1, 2], 4, 3, 1),           # chain id == n_chains
    ([0, 1, 2 ** 32 - 1], [0, 1, CP], 4, 3, 2),  # chain id far out, on a checkpoint op
    ([0, 1, 2], [0, 3, 1], 4, 3, 1),           # digest index == n_digests
    ([0, 1, 2], [0, 1, CP - 1], 4, 3, 2),      # just below the markers
    ([0], [0], 4, 0, 0),                       # a write into an empty table
    ([0, 9], [NULL, NULL], 4, 0, 1),           # a null write still names a chain
    ([0], [CP], 0, 0, 0),                      # no chains at all
])
def test_commit_plan_rejects_and_names_the_op(oc, od, n_chains, n_digests, bad):
    rc, *_, bad_op = plan_raw(oc, od, n_chains, n_digests)
    assert rc == _lib.MIRSHA_EINVAL and bad_op == bad
    with pytest.raises(MirshaError, match=f"op {bad}"):
        commit_plan(oc, od, n_chains, n_digests)


def test_commit_plan_null_arrays_and_limits():
    assert plan_raw([0, 1], [0, 1], 4, 3, null_chain=True)[0] == _lib.MIRSHA_EINVAL
    assert plan_raw([0, 1], [0, 1], 4, 3, null_digest=True)[0] == _lib.MIRSHA_EINVAL
    lib = _lib.load()
    oc = np.zeros(2, dtype=np.uint32)
    out = np.zeros(8, dtype=np.uint32)
    cnt = ctypes.c_uint32(0)
    args = (oc.ctypes.data, oc.ctypes.data, 2, 4, 3)
    # a NULL output array with ops to plan; NULL count outputs
    assert lib.mirsha_commit_plan(*args, None, out.ctypes.data, out.ctypes.data, cnt, cnt, cnt, None) == \
        _lib.MIRSHA_EINVAL
    assert lib.mirsha_commit_plan(*args, out.ctypes.data, None, out.ctypes.data, cnt, cnt, cnt, None) == \
        _lib.MIRSHA_EINVAL
    assert lib.mirsha_commit_plan(*args, out.ctypes.data, out.ctypes.data, None, cnt, cnt, cnt, None) == \
        _lib.MIRSHA_EINVAL
    assert lib.mirsha_commit_plan(*args, out.ctypes.data, out.ctypes.data, out.ctypes.data, None, cnt, cnt, None) == \
        _lib.MIRSHA_EINVAL
    # an entry's low 31 bits hold the digest index or the row
    assert plan_raw([0], [0], 4, FLAG + 1)[0] == _lib.MIRSHA_ERANGE
    assert plan_raw([0], [FLAG - 1], 4, FLAG)[0] == _lib.MIRSHA_OK


# ---- commit_programme ----------------------------------------------------------------

def d32(k):
    return hashlib.sha256(b"req%d" % k).digest()


def test_commit_programme_shares_the_table_between_nodes():
    commits = [Commit(batch=CommitBatch([d32(0), None, d32(1)])), Commit(checkpoint=Checkpoint(1)),
               Commit(batch=CommitBatch([b"", d32(2)])), Commit(batch=CommitBatch([])),
               Commit(checkpoint=Checkpoint(3))]
    table, oc, od = commit_programme(commits, 3)
    assert table.shape == (3, 32) and [r.tobytes() for r in table] == [d32(0), d32(1), d32(2)]
    prog = [0, NULL, 1, CP, NULL, 2, CP]
    assert od.tolist() == [p for p in prog for _ in range(3)]
    assert oc.tolist() == [0, 1, 2] * len(prog)
    table, oc, od = commit_programme([], 2)
    assert table.shape == (0, 32) and oc.size == 0 and od.size == 0
    with pytest.raises(ValueError):
        commit_programme([Commit()], 1)
    with pytest.raises(ValueError):
        commit_programme([Commit(batch=CommitBatch([]), checkpoint=Checkpoint())], 1)
    with pytest.raises(ValueError):
        commit_programme([Commit(batch=CommitBatch([b"short"]))], 1)


# ---- Processor plumbing --------------------------------------------------------------

def sha(parts):
    return hashlib.sha256(b"".join(parts)).digest()


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
        return FakeTicket(self.hash_slices(requests))

    def wait(self, ticket):
        return ticket.out

    def poll(self, ticket):
        return True


class FakeLog:
    """NodeState restated (recorder.go:186-256): one streaming hasher."""

    def __init__(self, calls=None):
        self.h = hashlib.sha256()
        self.cycles = []
        self.calls = calls

    def commit_cycle(self, commits):
        if self.calls is not None:
            self.calls.append("commit_cycle")
        self.cycles.append(len(commits))
        out = []
        for c in commits:
            if c.batch is not None:
                for d in c.batch.digests:
                    self.h.update(d or b"")
            else:
                out.append(self.h.digest())
                self.h = hashlib.sha256()
        return out


def cycle():
    reqs = [HashRequest(data=[b"a", b"bc"], origin=1), HashRequest(data=[b""], origin=2)]
    commits = [Commit(batch=CommitBatch([d32(0), d32(1)], seq_no=1)), Commit(checkpoint=Checkpoint(seq_no=1)),
               Commit(checkpoint=Checkpoint(seq_no=1)), Commit(batch=CommitBatch([None, d32(2)], seq_no=2)),
               Commit(checkpoint=Checkpoint(seq_no=2)), Commit(batch=CommitBatch([d32(3)], seq_no=3))]
    want = [hashlib.sha256(d32(0) + d32(1)).digest(), hashlib.sha256().digest(), hashlib.sha256(d32(2)).digest()]
    return reqs, commits, want


def check_results(res, reqs, commits, want):
    assert isinstance(res, ActionResults)
    assert [r.digest for r in res.digests] == [sha(q.data) for q in reqs]
    assert all(r.request is q for r, q in zip(res.digests, reqs))
    asked = [c for c in commits if c.checkpoint is not None]
    assert len(res.checkpoints) == len(asked) == len(want)
    for r, c, v in zip(res.checkpoints, asked, want):  # commit order, back-pointers
        assert isinstance(r, CheckpointResult)
        assert r.commit is c and r.checkpoint is c.checkpoint and r.value == v


@pytest.mark.parametrize("how", ["process", "submit", "pool", "pool_overlap"])
def test_checkpoints_in_commit_order_with_back_pointers(how):
    reqs, commits, want = cycle()
    eng = FakeEngine()
    log = FakeLog(eng.calls)
    actions = Actions(hash=reqs, commits=commits)
    if how == "process":
        res = Processor(engine=eng, log=log).process(actions)
    elif how == "submit":
        pending = Processor(engine=eng, log=log).submit(actions)
        assert log.cycles == [6]  # applied at submission
        res = pending.wait()
        assert pending.wait() is res
    elif how == "pool":
        res = ProcessorWorkPool(engine=eng, log=log).process(actions)
    else:
        ran = []
        res = ProcessorWorkPool(engine=eng, log=log).process(actions, overlap=lambda: ran.append(1))
        assert ran == [1]
    check_results(res, reqs, commits, want)
    assert log.cycles == [6]  # the whole cycle in ONE call to the log
    # the log carries on into the next cycle: d32(3) is still in the hasher
    more = Actions(commits=[Commit(checkpoint=Checkpoint(seq_no=3))])
    res2 = Processor(engine=eng, log=log).process(more)
    assert res2.digests == [] and [r.value for r in res2.checkpoints] == [hashlib.sha256(d32(3)).digest()]


@pytest.mark.parametrize("cls", [Processor, ProcessorWorkPool])
def test_commits_without_a_log_raise(cls):
    reqs, commits, _ = cycle()
    p = cls(engine=FakeEngine())
    with pytest.raises(RuntimeError, match="log"):
        p.process(Actions(hash=reqs, commits=commits))
    with pytest.raises(RuntimeError, match="log"):
        p.submit(Actions(commits=commits[:1]))


@pytest.mark.parametrize("with_log", [False, True])
def test_no_commits_changes_nothing(with_log):
    reqs, _, _ = cycle()
    eng = FakeEngine()
    log = FakeLog() if with_log else None
    assert Actions().commits == [] and Actions(hash=reqs).commits == []
    for p in (Processor(engine=eng, log=log), ProcessorWorkPool(engine=eng, log=log)):
        for res in (p.process(Actions(hash=reqs)), p.submit(Actions(hash=reqs)).wait()):
            assert res.checkpoints == []
            assert [r.digest for r in res.digests] == [sha(q.data) for q in reqs]
        empty = p.process(Actions())
        assert empty.digests == [] and empty.checkpoints == []
    if log is not None:
        assert log.cycles == []  # a cycle without commits never reaches the log


def test_a_log_that_miscounts_is_an_error():
    class Short(FakeLog):
        def commit_cycle(self, commits):
            return super().commit_cycle(commits)[:-1]

    _, commits, _ = cycle()
    with pytest.raises(RuntimeError, match="2 values for 3 checkpoints"):
        Processor(engine=FakeEngine(), log=Short()).process(Actions(commits=commits))
