"""A cycle's Commits in one call (mirsha_chains_commit): the commit loop of
Processor.Process (processor.go:145-168) over the device-resident checkpoint
chains.  Expected values come from hashlib streaming hashers, one per chain,
as NodeState.ActiveHash (testengine/recorder.go:186-256), and from the golden
fixtures; never from the code under test."""
import ctypes
import hashlib

import numpy as np
import pytest

from mirbft_amd import (Actions, Checkpoint, CheckpointChains, Commit, CommitBatch, DeviceLog, HashRequest,
                        MirshaError, Processor, ProcessorWorkPool, _lib, commit_plan, device_count, hashdata)

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


# ---- parity classes -------------------------------------------------------------------

def parity_classes():
    """(entry parity, writes before the first checkpoint, writes between two
    checkpoints or None for a single checkpoint, writes after the last)."""
    return [(odd, a, m, b) for odd in (0, 1) for a in range(4) for m in (None, 0, 1, 2, 3) for b in range(4)]


@pytest.mark.parametrize("together", [True, False], ids=["one_call", "one_call_per_chain"])
def test_parity_classes(engine, together):
    """Every entry parity x 0-3 writes before the first checkpoint x 0-3 after
    the last (x 0-3 between two checkpoints): as the lanes of ONE call, and
    each class as a lone lane in a call of its own.  The leftover state is
    checked by a later sum, and again after one more write."""
    rng = np.random.default_rng(21)
    classes = parity_classes()
    n = len(classes)
    ch = CheckpointChains(engine, n)
    ref = [hashlib.sha256() for _ in range(n)]
    table = table_of(rng, 16)
    odd = [c for c, cl in enumerate(classes) if cl[0]]
    first = table_of(rng, len(odd))
    ch.write(first, np.asarray(odd, dtype=np.uint32))  # the pending digest of an earlier call
    for row, c in zip(first, odd):
        ref[c].update(row.tobytes())
    programmes = []
    for c, (_, a, m, b) in enumerate(classes):
        w = lambda k: [int(x) for x in rng.integers(0, 16, k)]
        programmes.append((c, w(a) + [CP] + ([] if m is None else w(m) + [CP]) + w(b)))
    calls = [interleave(rng, programmes)] if together else [interleave(rng, [p]) for p in programmes]
    got = []
    want = []
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


# ---- empty checkpoints ----------------------------------------------------------------

def test_empty_checkpoints(engine):
    rng = np.random.default_rng(22)
    table = table_of(rng, 3)
    ch = CheckpointChains(engine, 3)
    # the very first op on a fresh chain (recorder_test.go:83), and two back to back
    got = values(ch.commit(table, [0, 1, 1, 1], [CP, 0, CP, CP]))
    assert got == [EMPTY, hashlib.sha256(table[0].tobytes()).digest(), EMPTY]
    assert sums(ch) == [EMPTY] * 3
    # a checkpoint as the last op: the next call starts the chain empty
    got = values(ch.commit(table, [2, 2, 2], [1, 2, CP]))
    assert got == [hashlib.sha256(table[1].tobytes() + table[2].tobytes()).digest()]
    got = values(ch.commit(table, [2, 2], [0, CP]))
    assert got == [hashlib.sha256(table[0].tobytes()).digest()]
    assert values(ch.commit(table, [2], [CP])) == [EMPTY]
    # an empty table: checkpoints and nulls only
    assert values(ch.commit(np.zeros((0, 32), np.uint8), [0, 0, 1], [NULL, CP, CP])) == [EMPTY, EMPTY]
    assert ch.commit(table, [], []).shape == (0, 32)
    ch.close()


# ---- widths -----------------------------------------------------------------------------

@pytest.mark.parametrize("n_active", [1, 63, 64, 65, 257, 300])
def test_widths(engine, n_active):
    """n_active chains with entries in one call (that many lanes): 1 to 40
    ops each, 0-3 checkpoints among them, any entry parity.  Between them idle
    chains, at least one in every 64 ids and so in every wave's range, with a
    state of their own that must not change: never named, or (0 entries)
    named by null writes only."""
    rng = np.random.default_rng(300 + n_active)
    n = n_active + n_active // 50 + 2
    idle = set(range(7, n, 50)) | {n - 1}
    active = [c for c in range(n) if c not in idle][:n_active]
    idle = [c for c in range(n) if c not in active]
    assert len(active) == n_active and idle
    assert all(any(c in idle for c in range(lo, min(lo + 64, n))) for lo in range(0, n, 64))
    ch = CheckpointChains(engine, n)
    ref = [hashlib.sha256() for _ in range(n)]
    pre_chain = np.asarray([c for c in range(n) if rng.random() < 0.5 or c in idle] * 1, dtype=np.uint32)
    pre_chain = np.concatenate([pre_chain, pre_chain[rng.random(pre_chain.size) < 0.3]])  # some get two: even
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
    act, efirst, ent, n_values = commit_plan(oc, od, n, 97)
    assert act.tolist() == active and n_values == int(np.count_nonzero(od == CP))
    got = values(ch.commit(table, oc, od))
    assert got == run_ref(ref, table, oc, od)
    assert sums(ch, np.asarray(idle, dtype=np.uint32)) == idle_before
    assert sums(ch) == [r.digest() for r in ref]
    ch.close()


# ---- shared table -----------------------------------------------------------------------

@pytest.mark.parametrize("n_nodes", [4, 100])
def test_shared_table(engine, n_nodes):
    """N nodes commit one batch: every chain writes the same rows of a table
    that is passed once, nulls interleaved, rows used out of order and more
    than once."""
    rng = np.random.default_rng(23)
    table = table_of(rng, 40)
    prog = [39, 0, NULL, 17, 17, 3, CP, NULL, NULL, 38, 2, 1, CP, 0, 39, 20, NULL]
    od = np.repeat(np.asarray(prog, dtype=np.uint32), n_nodes)
    oc = np.tile(np.arange(n_nodes, dtype=np.uint32), len(prog))
    ch = CheckpointChains(engine, n_nodes)
    ref = [hashlib.sha256() for _ in range(n_nodes)]
    got = values(ch.commit(table, oc, od))
    want = run_ref(ref, table, oc, od)
    assert got == want and len(set(got)) == 2 and len(got) == 2 * n_nodes
    assert sums(ch) == [r.digest() for r in ref]
    ch.close()


# ---- equivalence with the three-call form ------------------------------------------------

def random_cycle(rng, n, n_ops, n_digests):
    oc = rng.integers(0, n, n_ops).astype(np.uint32)
    od = rng.integers(0, n_digests, n_ops).astype(np.uint32)
    kind = rng.random(n_ops)
    od[kind < 0.1] = NULL
    od[kind > 0.9] = CP
    return oc, od


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


def test_equivalence_with_write_sum_reset(engine):
    rng = np.random.default_rng(24)
    n = 70
    a, b, mixed = (CheckpointChains(engine, n) for _ in range(3))
    ref = [hashlib.sha256() for _ in range(n)]
    for cycle in range(6):
        table = table_of(rng, 50)
        oc, od = random_cycle(rng, n, int(rng.integers(0, 400)), 50)
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


# ---- device form ------------------------------------------------------------------------

def test_commit_device_on_hashed_requests(engine):
    """Request digests written by hash_batch_device into a torch buffer are
    committed where they lie; the values equal the host form's on hashlib's
    digests of the same requests."""
    import torch

    rng = np.random.default_rng(25)
    n_req, n = 200, 5
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
    engine.hash_batch_device(d_arena.data_ptr(), arena.size, d_off.data_ptr(), d_len.data_ptr(), None, n_req,
                             d_out.data_ptr())
    oc, od = random_cycle(rng, n, 500, n_req)
    dev, hst = CheckpointChains(engine, n), CheckpointChains(engine, n)
    ref = [hashlib.sha256() for _ in range(n)]
    got = values(dev.commit_device(d_out.data_ptr(), n_req, oc, od))  # queued behind the hashing
    want = run_ref(ref, host, oc, od)
    assert got == want and len(want) > 10
    assert values(hst.commit(host, oc, od)) == want
    assert sums(dev) == sums(hst) == [r.digest() for r in ref]
    assert np.array_equal(d_out.cpu().numpy(), host)
    dev.close()
    hst.close()


# ---- validation -------------------------------------------------------------------------

def test_validation_failures_leave_the_states(engine):
    import torch

    rng = np.random.default_rng(26)
    n = 6
    ch = CheckpointChains(engine, n)
    table = table_of(rng, 8)
    ch.write(table[:5], np.asarray([0, 1, 1, 3, 5], dtype=np.uint32))
    before = sums(ch)
    good_c = np.asarray([0, 1, 2, 3], dtype=np.uint32)
    good_d = np.asarray([0, CP, 1, NULL], dtype=np.uint32)

    def rc_of(call, tab, n_dig, oc, od, n_ops, out_ptr="own", count=True):
        out = np.zeros((8, 32), dtype=np.uint8)
        k = ctypes.c_uint32(77)
        rc = call(engine.ctx, ch.handle, tab, n_dig, None if oc is None else oc.ctypes.data,
                  None if od is None else od.ctypes.data, n_ops, out.ctypes.data if out_ptr == "own" else out_ptr,
                  ctypes.byref(k) if count else None)
        assert not out.any()
        return rc

    lib = engine._lib
    host = lib.mirsha_chains_commit
    tab = table.ctypes.data
    bad = [
        ("chain id", lambda: rc_of(host, tab, 8, np.asarray([0, n], dtype=np.uint32), good_d[:2].copy(), 2)),
        ("digest index", lambda: rc_of(host, tab, 8, good_c, np.asarray([0, CP, 8, 1], dtype=np.uint32), 4)),
        ("below the markers", lambda: rc_of(host, tab, 8, good_c, np.asarray([0, CP - 1, 1, 1], np.uint32), 4)),
        ("NULL op_chain", lambda: rc_of(host, tab, 8, None, good_d, 4)),
        ("NULL op_digest", lambda: rc_of(host, tab, 8, good_c, None, 4)),
        ("NULL table", lambda: rc_of(host, None, 8, good_c, good_d, 4)),
        ("NULL values_out", lambda: rc_of(host, tab, 8, good_c, good_d, 4, out_ptr=None)),
        ("NULL n_values_out", lambda: rc_of(host, tab, 8, good_c, good_d, 4, count=False)),
    ]
    d_tab = torch.from_numpy(np.concatenate([table.reshape(-1), np.zeros(32, np.uint8)])).cuda()
    torch.cuda.synchronize()
    bad.append(("misaligned device table",
                lambda: rc_of(lib.mirsha_chains_commit_device, d_tab.data_ptr() + 4, 8, good_c, good_d, 4)))
    for name, call in bad:
        assert call() == _lib.MIRSHA_EINVAL, name
        assert sums(ch) == before, name
    with pytest.raises(MirshaError, match=r"op_chain\[1\] = 6 >= 6"):
        ch.commit(table, [0, 6], [0, 1])
    with pytest.raises(MirshaError, match=r"op_digest\[2\] = 8 >= 8"):
        ch.commit(table, [0, 1, 2], [0, 1, 8])
    assert sums(ch) == before
    if device_count() > 1:  # chains of another device
        from mirbft_amd import Engine

        other = Engine(1)
        theirs = CheckpointChains(other, n)
        k = ctypes.c_uint32(0)
        out = np.zeros((4, 32), dtype=np.uint8)
        assert host(engine.ctx, theirs.handle, tab, 8, good_c.ctypes.data, good_d.ctypes.data, 4, out.ctypes.data,
                    ctypes.byref(k)) == _lib.MIRSHA_EINVAL
        assert sums(theirs) == [EMPTY] * n
        theirs.close()
        other.close()
    # the same arguments, valid: n_ops == 0 is fine with NULL arrays
    assert rc_of(host, None, 0, None, None, 0) == _lib.MIRSHA_OK
    assert sums(ch) == before
    ch.close()


# ---- Processor --------------------------------------------------------------------------

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


@pytest.mark.parametrize("cls", [Processor, ProcessorWorkPool])
def test_processor_cycle_with_hashes_and_commits(engine, cls):
    rng = np.random.default_rng(27)
    log = DeviceLog(engine)
    p = cls(engine=engine, log=log)
    state = NodeState()
    seq = 0
    for cycle in range(4):
        reqs = [HashRequest(data=[rng.bytes(int(k)) for k in rng.integers(0, 90, 3)], origin=i) for i in range(25)]
        commits = []
        for _ in range(7):
            seq += 1
            digests = [None if rng.random() < 0.15 else rng.bytes(32) for _ in range(int(rng.integers(0, 6)))]
            commits.append(Commit(batch=CommitBatch(digests, seq_no=seq)))
            if seq % 3 == 0:  # a checkpoint in the middle of the list
                commits.append(Commit(checkpoint=Checkpoint(seq_no=seq)))
        if cycle == 2:
            commits = []  # a cycle without commits
        res = p.process(Actions(hash=reqs, commits=commits))
        assert [r.digest for r in res.digests] == [sha(q.data) for q in reqs]
        assert all(r.request is q for r, q in zip(res.digests, reqs))
        asked = [c for c in commits if c.checkpoint is not None]
        assert [r.value for r in res.checkpoints] == state.commit(commits)
        assert [r.commit for r in res.checkpoints] == asked
        assert all(r.checkpoint is c.checkpoint for r, c in zip(res.checkpoints, asked))
    assert log.chains.sum([0])[0].tobytes() == state.active.digest()
    log.close()


def test_testengine_log_of_four_nodes_on_golden_digests(engine, layouts):
    """The golden checkpoint chain (60 testengine requests committed in
    batches of 5, checkpoints after 20, 40 and 60 and one more on the empty
    state) driven through a 4-node DeviceLog: one commit call per cycle, the
    table passed once for the four nodes."""
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
    p = Processor(engine=engine, log=log)
    reqs = [HashRequest(data=hashdata.request_hash_data(r["client"], r["req_no"],
                                                        hashdata.testengine_request_payload(r["client"], r["req_no"])))
            for r in layouts["testengine_requests"][:40]]
    # two cycles: the cut falls between a batch and its checkpoint
    cut = 9
    got = []
    for part in (commits[:cut], commits[cut:]):
        res = p.process(Actions(hash=reqs, commits=part))
        assert [r.digest.hex() for r in res.digests] == [r["sha256"] for r in layouts["testengine_requests"][:40]]
        got += [r.value for r in res.checkpoints]
        assert log.values.shape == (len(res.checkpoints), 4, 32)
        for node in range(4):  # every node's chain holds the same value
            assert [v.tobytes() for v in log.values[:, node]] == [r.value for r in res.checkpoints]
    assert got == want
    assert sums(log.chains) == [EMPTY] * 4
    log.close()


# ---- C++ host mirror --------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, 2], ids=["process", "submit_wait"])
def test_cpp_host_mirror_commit_loop(flags):
    """mirbft::Processor with a 3-node mirbft::DeviceLog (mirbft_amd/host): the
    same cycle, batches with null requests and a checkpoint mid-list; the C
    entry itself checks the order and the back-pointers."""
    rng = np.random.default_rng(28)
    host = ctypes.CDLL(_lib.HOST_LIB_PATH)
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
